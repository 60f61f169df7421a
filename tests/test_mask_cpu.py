"""CPU: the host side of training on incomplete patients: the missing-value pattern the GPU tests rely on, the
fp64 oracle's identities, OsteosarcomaDataset(incomplete=...), and every refusal -- each a ValueError before any device work."""
import numpy as np
import pandas as pd
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.train import OsteosarcomaDataset, Trainer, prepare_data
from helpers import config
from loss_helpers import Fp64Oracle, inputs
from mask_helpers import (FULL_ROW, PROLOGUE_SHAPES, SHAPES, MaskedOracle, MixupMaskedOracle, mask_pattern, mix, q_sample_fp32, with_nan,
                          zero_fill)

SM_DIMS, SM_H, SM_N = (8, 24, 8, 3), [32, 64, 32], 16


@pytest.mark.parametrize("name", list(SHAPES) + list(PROLOGUE_SHAPES))
def test_mask_pattern_has_every_property(name):
    """A condition of the GPU file: no case there can run without a masked tail, a fully observed row or an all-missing row."""
    dims, n = (SHAPES[name]["dims"], SHAPES[name]["n"]) if name in SHAPES else PROLOGUE_SHAPES[name]
    mut, expr, pw, _ = dims
    D = mut + expr + pw
    miss = mask_pattern(n, dims)
    assert miss.shape == (n, D) and miss.dtype == torch.bool
    assert torch.equal(miss, mask_pattern(n, dims)), "not deterministic"
    assert miss[0].all(), "row 0 is not entirely missing"
    assert not miss[FULL_ROW].any(), "no fully observed row"
    tail = D % 32 + 4
    assert miss[n - 1, D - tail:].all(), "the last row's tail columns are observed"
    assert not miss[n - 1].all() or n - 1 == 0, "the last row has nothing observed"
    no_expr = miss[:, mut:mut + expr].all(dim=1)
    frac_rows = float(no_expr[2:].double().mean())
    assert 0.1 <= frac_rows <= 0.6 and int(no_expr.sum()) >= 2, f"{frac_rows:.2f} of the rows lack the expression block"
    scattered = float(miss[~no_expr][:, :mut].double().mean()) if mut else 0.1
    assert 0.03 <= scattered <= 0.25, f"scattered fraction {scattered:.3f}"
    assert (~miss).any(dim=0).all(), "a column is never observed"


def _small(seed=17):
    sd, x, cond, t, noise, injected = inputs(SM_DIMS, SM_H, SM_N, seed=seed)
    return sd, x, cond, t, noise, injected


def test_oracle_without_nan_is_the_unmasked_oracle_exactly():
    sd, x, cond, t, noise, injected = _small()
    table = torch.rand(1000, generator=torch.Generator().manual_seed(4)) + 0.05
    for kind, delta, w in (("l2", 1.0, None), ("l1", 1.0, table), ("huber", 0.3, table)):
        ref = Fp64Oracle(sd, x, cond, t, noise, SM_H, injected, 0.2).loss_and_grads(kind, delta, w)
        got = MaskedOracle(sd, x, cond, t, noise, SM_H, injected, 0.2).loss_and_grads(kind, delta, w)
        assert got[0] == ref[0]
        for k in ref[1]:
            assert torch.equal(got[1][k], ref[1][k]), k


def test_oracle_all_missing_batch_is_zero():
    sd, x, cond, t, noise, injected = _small()
    nan = torch.full_like(x, float("nan"))
    for ptype in ("epsilon", "v_prediction", "sample"):
        loss, grads = MaskedOracle(sd, nan, cond, t, noise, SM_H, injected, 0.2).loss_and_grads("huber", 0.5, None, ptype)
        assert loss == 0.0
        assert all(bool((g == 0).all()) for g in grads.values())


def test_oracle_masked_elements_do_not_count():
    """The masked loss is the sum over the observed elements alone, divided by n D; changing a value under the mask changes nothing."""
    sd, x, cond, t, noise, injected = _small()
    miss = mask_pattern(SM_N, SM_DIMS)
    orc = MaskedOracle(sd, with_nan(x, miss), cond, t, noise, SM_H, injected, 0.2)
    loss, grads = orc.loss_and_grads("l2", 1.0, None, "v_prediction")
    x2 = torch.where(miss, x + 5.0, x)
    loss2, _ = MaskedOracle(sd, with_nan(x2, miss), cond, t, noise, SM_H, injected, 0.2).loss_and_grads("l2", 1.0, None, "v_prediction")
    assert loss == loss2 and loss > 0
    xt, tgt = q_sample_fp32(with_nan(x, miss), t, noise, "v_prediction")
    assert torch.equal(torch.isnan(tgt), miss) and torch.isfinite(xt).all()
    d = (orc.pred.detach() - zero_fill(tgt).double())[~miss]
    assert abs(float((d * d).sum()) / miss.numel() - loss) <= 1e-6 * loss


def test_mixup_element_is_observed_iff_both_parents_are():
    sd, x, cond, t, noise, injected = _small()
    miss = mask_pattern(SM_N, SM_DIMS)
    perm = torch.randperm(SM_N, generator=torch.Generator().manual_seed(3))
    idx = torch.arange(SM_N)
    xm, cm = mix(with_nan(x, miss), cond, idx, perm, 0.3)
    assert torch.equal(torch.isnan(xm), miss | miss[perm])
    assert torch.isfinite(cm).all()
    orc = MixupMaskedOracle(sd, with_nan(x, miss), cond, idx, perm, 0.3, t, noise, SM_H)
    assert torch.equal(orc.observed, ~(miss | miss[perm]))


# ---- OsteosarcomaDataset(incomplete=...) ------------------------------------------------------------------------------------------
def _frames():
    rng = np.random.default_rng(0)
    mut = pd.DataFrame(rng.integers(0, 2, (5, 3)).astype(np.float32), index=["p1", "p2", "p3", "p4", "p9"], columns=list("abc"))
    expr = pd.DataFrame(rng.normal(size=(3, 4)).astype(np.float32), index=["p2", "p3", "p5"], columns=list("wxyz"))
    pw = pd.DataFrame(rng.normal(size=(4, 2)).astype(np.float32), index=["p3", "p2", "p4", "p5"], columns=["k1", "k2"])
    clin = pd.DataFrame({"submitter_id": ["p1", "p2", "p3", "p4", "p5", "p7"], "age": [1.0, 2.0, np.nan, 4.0, 5.0, 7.0],
                         "survival_days": [10.0, 20.0, 30.0, np.nan, 50.0, 70.0]})
    return mut, expr, pw, clin


def test_dataset_drop_is_the_intersection():
    mut, expr, pw, clin = _frames()
    default = OsteosarcomaDataset(mut, expr, pw, clin, ["age"])
    drop = OsteosarcomaDataset(mut, expr, pw, clin, ["age"], incomplete="drop")
    assert default.data.shape == (2, 9) and torch.isfinite(default.data).all()
    want = np.concatenate([mut.loc[["p2", "p3"]].values, expr.loc[["p2", "p3"]].values, pw.loc[["p2", "p3"]].values], axis=1)
    assert np.array_equal(default.data.numpy(), want)
    for k in ("data", "conditions", "survival_days"):
        assert torch.equal(getattr(default, k), getattr(drop, k))
    assert default.conditions[:, 0].tolist() == [2.0, 0.0]


def test_dataset_keep_is_the_union_with_nan_blocks():
    mut, expr, pw, clin = _frames()
    ds = OsteosarcomaDataset(mut, expr, pw, clin, ["age"], incomplete="keep")
    rows = ["p1", "p2", "p3", "p4", "p5"]                   # the union, minus p9 (no clinical row); p7 has no features
    assert ds.data.shape == (5, 9) and len(ds) == 5
    for i, p in enumerate(rows):
        for block, lo, hi in ((mut, 0, 3), (expr, 3, 7), (pw, 7, 9)):
            got = ds.data[i, lo:hi]
            if p in block.index:
                assert np.array_equal(got.numpy(), block.loc[p].values), (p, lo)
            else:
                assert torch.isnan(got).all(), (p, lo)
    assert torch.isfinite(ds.conditions).all() and torch.isfinite(ds.survival_days).all()
    assert ds.conditions[:, 0].tolist() == [1.0, 2.0, 0.0, 4.0, 5.0]
    blocks = torch.cat([ds.mutations, ds.expression, ds.pathways], dim=1)
    assert torch.equal(torch.isnan(ds.data), torch.isnan(blocks)) and torch.equal(zero_fill(ds.data), zero_fill(blocks))
    item = ds[0]
    assert set(item) == {"data", "conditions", "survival"}
    with pytest.raises(ValueError):
        OsteosarcomaDataset(mut, expr, pw, clin, ["age"], incomplete="zero")


def test_prepare_data_keeps_incomplete_patients_under_the_mask(tmp_path):
    mut, expr, pw, clin = _frames()
    clin["event_occurred"] = 1.0
    mut.to_csv(tmp_path / "mutation_matrix_aligned.csv")
    expr.to_csv(tmp_path / "expression_matrix_aligned.csv")
    pw.to_csv(tmp_path / "pathway_scores.csv")
    clin.to_csv(tmp_path / "clinical_aligned.csv", index=False)

    def rows(**training):
        conf = {"data": {"processed_dir": str(tmp_path)}, "model": {},
                "training": dict({"val_split": 0.0, "random_seed": 1, "batch_size": 1}, **training)}
        train_loader, _, _ = prepare_data(conf)
        return len(train_loader.dataset)

    assert rows() == 2 and rows(missing_values="mask") == 5
    with pytest.raises(ValueError):
        rows(missing_values="zero")


# ---- config validation and refusals -----------------------------------------------------------------------------------------------
def _conf(tmp_path, **training):
    conf = config(SM_H)
    conf["training"] = dict({"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 10, "min_delta": 1e-4,
                             "augmentation": {"mixup_alpha": 0.0}, "save_dir": str(tmp_path), "num_epochs": 1, "save_frequency": 10,
                             "val_split": 0.2, "random_seed": 42, "batch_size": 16}, **training)
    return conf


def _model(conf):
    mut, expr, pw, cd = SM_DIMS
    return BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)


def test_model_reads_missing_values_from_the_config(tmp_path):
    assert _model(config(SM_H)).missing_values is None
    assert _model(_conf(tmp_path)).missing_values is None
    assert _model(_conf(tmp_path, missing_values="mask")).missing_values == "mask"
    for bad in ("zero", "Mask", True, 0):
        with pytest.raises(ValueError):
            _model(_conf(tmp_path, missing_values=bad))


def _loader(data):
    ds = object.__new__(OsteosarcomaDataset)
    ds.data, ds.conditions, ds.survival_days = data, torch.zeros(data.shape[0], SM_DIMS[3]), torch.zeros(data.shape[0])
    return torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0)


def test_trainer_refusals_come_before_any_device_work(tmp_path, monkeypatch):
    """Each of these is a ValueError of the constructor; the model is never moved to a device (which would fail here or not, but must
    not be reached)."""
    moved = []
    monkeypatch.setattr(BiologyAwareDiffusionModel, "to", lambda self, *a, **k: moved.append(a) or (_ for _ in ()).throw(AssertionError("device")))
    good = _loader(torch.randn(8, sum(SM_DIMS[:3])))

    def build(model=None, loader=good, **training):
        conf = _conf(tmp_path, **training)
        return Trainer(model if model is not None else _model(conf), loader, loader, conf, device="cuda")

    with pytest.raises(ValueError, match="missing_values"):
        build(missing_values="zero")
    with pytest.raises(ValueError, match="bound"):
        build(missing_values="mask", validation_metric="bound")
    with pytest.raises(ValueError, match="dp"):
        build(missing_values="mask", dp={"max_grad_norm": 1.0, "noise_multiplier": 1.0})
    cons = _model(_conf(tmp_path))
    cons.set_constraints([[0, 1, 9]], pathway_weight=0.5)
    with pytest.raises(ValueError, match="constraint"):
        build(model=cons, missing_values="mask")

    class Cvae(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.vae = torch.nn.Linear(2, 2)

    with pytest.raises(ValueError, match="cVAE"):
        build(model=Cvae(), missing_values="mask")
    inf = torch.randn(8, sum(SM_DIMS[:3]))
    inf[3, 5] = float("inf")
    with pytest.raises(ValueError, match="Inf"):
        build(loader=_loader(inf), missing_values="mask")
    # the model's own attribute is followed when the training section does not name the key
    m = _model(_conf(tmp_path))
    m.missing_values = "mask"
    with pytest.raises(ValueError, match="bound"):
        build(model=m, validation_metric="bound")
    assert not moved
    # zero constraint weights and NaN data pass every check: the constructor reaches the device move
    zero = _model(_conf(tmp_path))
    zero.set_constraints([[0, 1, 9]], pathway_weight=0.0, mutexpr_weight=0.0)
    nan = torch.randn(8, sum(SM_DIMS[:3]))
    nan[2, :7] = float("nan")
    with pytest.raises(AssertionError, match="device"):
        build(model=zero, loader=_loader(nan), missing_values="mask")
    assert zero.missing_values == "mask"


def test_observed_fraction_is_logged(tmp_path, caplog):
    import logging
    nan = torch.randn(8, 40)
    nan[:2] = float("nan")
    with caplog.at_level(logging.INFO):
        Trainer._check_incomplete_data(_loader(nan))
    assert any("0.7500" in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records]


def test_set_loss_mask_rejects_a_null_handle():
    lib = L.lib()
    assert lib.osd_set_loss_mask(None, 1) == L.OSD_EINVAL
    assert L.last_error()
    assert L.OSD_TP_MASKED == 1 << 14
