"""CPU: the weight-averaging (EMA) feature's host side -- the two new C-ABI entry points and their argument checks (made before any
device call), ParamEMA's decay schedule and state dict, the Trainer's config validation and load_trained_model's choice between
the averaged weights and the last iterate."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, _lib as L, load_trained_model
from osteosarcoma_diffusionmodel_amd.train import FlatParams, ParamEMA, Trainer
from helpers import SM, SM_H, config

ROOT = Path(__file__).resolve().parent.parent
NEW = ("osd_clip_adamw_ema_step", "osd_nn_clip_adamw_ema_step")


def test_new_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "osdiff.h").read_text(), flags=re.S)
    lib = L.lib()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", header), f"{name} is not declared in include/osdiff.h"
        assert hasattr(lib, name), f"libosdiff.so does not export {name}"
        assert name in L.exported_symbols()
    # one more pointer (ema) and one more double (ema_decay) than the plain step
    for plain, ema in (("osd_clip_adamw_step", NEW[0]), ("osd_nn_clip_adamw_step", NEW[1])):
        a, b = L._SIGNATURES[plain][1], L._SIGNATURES[ema][1]
        assert len(b) == len(a) + 2
        assert b.count(C.c_void_p) == a.count(C.c_void_p) + 1 and b.count(C.c_double) == a.count(C.c_double) + 1
    assert lib.osd_version() == 100


def _nn_call(ema, decay, param=64):
    """osd_nn_clip_adamw_ema_step with dummy non-NULL addresses: an argument error must return before anything is dereferenced."""
    p = C.c_void_p
    return L.lib().osd_nn_clip_adamw_ema_step(p(0), 0, p(64), p(param), p(64), p(64), p(64), p(ema), 16, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1,
                                              decay, p(0))


@pytest.mark.parametrize("ema, decay", [(0, 0.5), (64, -0.1), (64, 1.5), (64, float("nan"))])
def test_ema_step_rejects_bad_arguments_before_any_device_call(ema, decay):
    assert _nn_call(ema, decay) == L.OSD_EINVAL
    assert L.last_error()
    p = C.c_void_p
    rc = L.lib().osd_clip_adamw_ema_step(p(64), p(64), p(64), p(64), p(64), p(ema), 16, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1, decay, p(0))
    assert rc == L.OSD_EINVAL


def test_ema_step_null_param_is_still_einval():
    assert _nn_call(64, 0.5, param=0) == L.OSD_EINVAL


def _tiny():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 2))
    return m, FlatParams(m)


def test_decay_at():
    m, flat = _tiny()
    e = ParamEMA(m, flat, 0.999)
    assert e.warmup and e.num_updates == 0
    assert e.decay_at(1) == 2.0 / 11.0
    assert e.decay_at(10) == 11.0 / 20.0
    # k = 1000 is still inside the warm-up at decay 0.999: (1 + k) / (10 + k) = 1001 / 1010 < 0.999; the cap is reached at k = 8990
    assert e.decay_at(1000) == 1001.0 / 1010.0
    assert e.decay_at(8989) == 8990.0 / 8999.0 < 0.999 and e.decay_at(8990) == 0.999 and e.decay_at(10 ** 6) == 0.999
    assert ParamEMA(m, flat, 0.99).decay_at(1000) == 0.99          # ... and at decay 0.99 it is over by k = 1000
    ks = np.arange(1, 20000)
    d = np.array([e.decay_at(int(k)) for k in ks])
    assert np.all(np.diff(d) >= 0) and d.max() == 0.999 and np.all(d == np.minimum(0.999, (1.0 + ks) / (10.0 + ks)))
    e2 = ParamEMA(m, flat, 0.999, warmup=False)
    assert [e2.decay_at(k) for k in (1, 10, 1000)] == [0.999] * 3
    for bad in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            ParamEMA(m, flat, bad)


def test_param_ema_state_dict_round_trip():
    m, flat = _tiny()
    e = ParamEMA(m, flat, 0.99)
    assert e.shadow.data_ptr() != flat.flat.data_ptr() and torch.equal(e.shadow, flat.flat)
    with torch.no_grad():
        e.shadow.add_(1.0)                      # the average moved away from the live weights
        m[1].running_mean.fill_(0.25)           # a buffer: not averaged, taken from the live model
    e.num_updates = 7
    sd = e.state_dict()
    assert list(ParamEMA.model_state(sd)) == list(m.state_dict()) and set(sd) - set(m.state_dict()) == {"decay", "warmup", "num_updates"}
    assert (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.99, True, 7)
    live = m.state_dict()
    params = {k for k, _ in m.named_parameters()}
    for k, v in ParamEMA.model_state(sd).items():
        assert torch.equal(v, live[k] + 1.0 if k in params else live[k]), k
    m2, flat2 = _tiny()
    e2 = ParamEMA(m2, flat2, 0.99)
    e2.load_state_dict(sd)
    assert torch.equal(e2.shadow, e.shadow) and e2.num_updates == 7
    with pytest.raises(KeyError):
        e2.load_state_dict({"decay": 0.99})


def _train_conf(tmp_path, **extra):
    conf = config(SM_H, p=0.0)
    conf["training"] = {"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.0},
                        "save_dir": str(tmp_path), "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": 16,
                        **extra}
    return conf


@pytest.mark.parametrize("bad", [1.0, -0.5])
def test_trainer_rejects_ema_decay_outside_open_unit_interval(tmp_path, bad):
    conf = _train_conf(tmp_path, ema_decay=bad)
    m = BiologyAwareDiffusionModel(config=conf, **SM)
    with pytest.raises(ValueError, match="ema_decay"):
        Trainer(m, [], [], conf, device="cuda")          # raised before the model is moved: no device needed


@pytest.fixture()
def checkpoints(tmp_path):
    """Two hand-built checkpoint files (with and without ema_state_dict) and the config that finds the feature dims."""
    conf = _train_conf(tmp_path)
    conf["data"] = {"processed_dir": str(tmp_path)}
    for fname, w in (("mutation_matrix_aligned.csv", SM["mutation_dim"]), ("expression_matrix_aligned.csv", SM["expression_dim"]),
                     ("pathway_scores.csv", SM["pathway_dim"])):
        pd.DataFrame(np.zeros((1, w)), index=["row0"], columns=[f"c{i}" for i in range(w)]).to_csv(tmp_path / fname)
    torch.manual_seed(3)
    m = BiologyAwareDiffusionModel(config=conf, **SM)
    last = {k: v.clone() for k, v in m.state_dict().items()}
    params = {k for k, _ in m.named_parameters()}
    avg = {k: (v + 0.5 if k in params else v.clone()) for k, v in last.items()}
    base = {"epoch": 4, "model_state_dict": last, "optimizer_state_dict": {}, "val_loss": 0.5, "config": conf}
    torch.save(dict(base, ema_state_dict=dict(avg, decay=0.99, warmup=True, num_updates=12)), tmp_path / "with.pt")
    torch.save(base, tmp_path / "without.pt")
    return conf, tmp_path, last, avg


def _same(model, sd):
    got = model.state_dict()
    return list(got) == list(sd) and all(torch.equal(got[k], sd[k]) for k in sd)


def test_load_trained_model_picks_the_weights(checkpoints):
    conf, d, last, avg = checkpoints
    assert _same(load_trained_model(d / "with.pt", conf, "cpu"), avg)                        # None: the average when it is there
    assert _same(load_trained_model(d / "with.pt", conf, "cpu", use_ema=None), avg)
    assert _same(load_trained_model(d / "with.pt", conf, "cpu", use_ema=True), avg)
    assert _same(load_trained_model(d / "with.pt", conf, "cpu", use_ema=False), last)
    assert _same(load_trained_model(d / "without.pt", conf, "cpu"), last)                     # None: falls back to the last iterate
    assert _same(load_trained_model(d / "without.pt", conf, "cpu", use_ema=False), last)
    with pytest.raises(KeyError):
        load_trained_model(d / "without.pt", conf, "cpu", use_ema=True)
    assert not load_trained_model(d / "with.pt", conf, "cpu").training


def test_load_trained_model_logs_which_weights(checkpoints, caplog):
    conf, d, _, _ = checkpoints
    with caplog.at_level("INFO", logger="osteosarcoma_diffusionmodel_amd.generate"):
        load_trained_model(d / "with.pt", conf, "cpu")
        assert "EMA weights" in caplog.text
        caplog.clear()
        load_trained_model(d / "with.pt", conf, "cpu", use_ema=False)
        assert "last iterate" in caplog.text and "Loaded the EMA weights" not in caplog.text
