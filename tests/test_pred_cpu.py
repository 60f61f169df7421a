"""Host: the prediction types (epsilon | v_prediction | sample) -- the step tables folded for each type against the unfolded step, the
three min-SNR forms, the argument checks, the checkpoint's type against the config's, and the C ABI's declarations.
tests/test_gpu_pred.py holds the device to the float64 oracles of tests/pred_helpers.py."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import objective as OB
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table, ddim_timesteps, ddim_x0_table
from osteosarcoma_diffusionmodel_amd.diffusion import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd.generate import checkpoint_prediction_type, load_trained_model
from helpers import SM, SM_H, config
from pred_helpers import PREDICTIONS, min_snr64, pq

ROOT = Path(__file__).resolve().parent.parent
T = 100
EPS32 = 2.0 ** -24          # half an ulp, relative: one rounding to fp32


def _bufs(T_=T):
    return O.schedule_buffers("cosine", T_)


@pytest.mark.parametrize("S", [1, 10, T])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_epsilon_tables_are_todays_bits(S, eta):
    ab = _bufs()["alphas_cumprod"]
    taus = ddim_timesteps(T, S)
    tau0, c0 = ddim_step_table(ab, taus, eta)
    tau1, c1 = ddim_step_table(ab, taus, eta, prediction="epsilon")
    assert np.array_equal(tau0, tau1) and c0.tobytes() == c1.tobytes()
    assert ddim_x0_table(ab, taus, eta).tobytes() == ddim_x0_table(ab, taus, eta, prediction="epsilon").tobytes()
    # ... and what the expressions of the parent commit give: A = sqrt(abar'/abar), B = dir - sqrt(abar') sqrt(1 - abar)/sqrt(abar)
    a64 = ab.float().double().numpy()
    for s in range(S):
        a, ap = a64[taus[s]], (a64[taus[s - 1]] if s > 0 else 1.0)
        sigma = eta * math.sqrt((1 - ap) / (1 - a)) * math.sqrt(max(1 - a / ap, 0.0))
        assert c0[s, 0] == np.float32(math.sqrt(ap / a))
        assert c0[s, 1] == np.float32(math.sqrt(max(1 - ap - sigma * sigma, 0.0)) - math.sqrt(ap) * math.sqrt(1 - a) / math.sqrt(a))


@pytest.mark.parametrize("prediction", PREDICTIONS)
@pytest.mark.parametrize("S", [1, 10, T])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_folded_row_reproduces_the_unfolded_step(prediction, S, eta):
    """On random float64 (x, out, z): A x + B out + C z against x0^ = P x + Q out, then x' = sqrt(abar') x0^ + dir (x - sqrt(abar) x0^)/
    sqrt(1 - abar) + sigma z, to 1e-6 relative (the row is rounded to fp32 once); E P + F = A and E Q = B within one fp32 rounding."""
    bufs = _bufs()
    ab = bufs["alphas_cumprod"]
    kw = dict(sqrt_alphas_cumprod=bufs["sqrt_alphas_cumprod"], sqrt_one_minus_alphas_cumprod=bufs["sqrt_one_minus_alphas_cumprod"])
    taus = ddim_timesteps(T, S)
    _, coef = ddim_step_table(ab, taus, eta, prediction, **kw)
    x0c = ddim_x0_table(ab, taus, eta, prediction, **kw)
    assert coef.dtype == np.float32 and x0c.dtype == np.float32 and np.isfinite(coef).all() and np.isfinite(x0c).all()
    # E, F and C do not depend on the type
    eps_x0c = ddim_x0_table(ab, taus, eta)
    assert np.array_equal(x0c[:, 2:], eps_x0c[:, 2:]) and np.array_equal(coef[:, 2], ddim_step_table(ab, taus, eta)[1][:, 2])
    # the buffers are optional: without them a and b are fp32 square roots of the fp32 abar, the model's buffers up to their last bit
    assert np.allclose(ddim_step_table(ab, taus, eta, prediction)[1], coef, rtol=4 * EPS32, atol=1e-9)
    a64 = ab.float().double()
    sa, sb = bufs["sqrt_alphas_cumprod"].float().double(), bufs["sqrt_one_minus_alphas_cumprod"].float().double()
    g = torch.Generator().manual_seed(3)
    x, out, z = (torch.randn(64, dtype=torch.float64, generator=g) for _ in range(3))
    c64, t64 = torch.from_numpy(coef).double(), torch.from_numpy(x0c).double()
    for s in range(S):
        a, ap = a64[taus[s]], (a64[taus[s - 1]] if s > 0 else torch.tensor(1.0, dtype=torch.float64))
        P, Q = pq(prediction, sa[taus[s]], sb[taus[s]])
        sigma = eta * torch.sqrt((1 - ap) / (1 - a)) * torch.sqrt(torch.clamp(1 - a / ap, min=0.0))
        direction = torch.sqrt(torch.clamp(1 - ap - sigma ** 2, min=0.0))
        x0 = P * x + Q * out
        ref = torch.sqrt(ap) * x0 + direction * (x - torch.sqrt(a) * x0) / torch.sqrt(1 - a) + sigma * z
        got = c64[s, 0] * x + c64[s, 1] * out + c64[s, 2] * z
        scale = (c64[s, 0].abs() * x.abs() + c64[s, 1].abs() * out.abs() + c64[s, 2].abs() * z.abs()).max().item()
        assert (got - ref).abs().max().item() <= 1e-6 * scale, (s, (got - ref).abs().max().item(), scale)
        # the unfolded table folds back: each of P, Q, E, F and A, B is one rounding of its float64 value
        E, Fc = t64[s, 2].item(), t64[s, 3].item()
        A, B = (E * t64[s, 0] + Fc).item(), (E * t64[s, 1]).item()
        mag_a = abs(E * t64[s, 0].item()) + abs(Fc)
        assert abs(A - coef[s, 0]) <= 4 * EPS32 * mag_a + 1e-45, (s, A, coef[s, 0])
        assert abs(B - coef[s, 1]) <= 4 * EPS32 * abs(B) + 1e-45, (s, B, coef[s, 1])
        assert x0c[s, 0] == np.float32(P.item()) and x0c[s, 1] == np.float32(Q.item())
    assert x0c[0, 2] == 1.0 and x0c[0, 3] == 0.0 and coef[0, 0] == x0c[0, 0] and coef[0, 1] == x0c[0, 1]      # the last step returns x0^


def test_v_gain_is_bounded_where_epsilons_is_not():
    """What the types are for: the larger of |P|, |Q| of x0^ = P x + Q out at the noisy end of the cosine T = 1000 schedule."""
    bufs = _bufs(1000)
    a, b = bufs["sqrt_alphas_cumprod"].double()[-1], bufs["sqrt_one_minus_alphas_cumprod"].double()[-1]
    gains = {p: max(abs(float(v)) for v in pq(p, a, b)) for p in ("epsilon",) + PREDICTIONS}
    assert gains["epsilon"] > 1e4 and gains["v_prediction"] <= 1.0 and gains["sample"] == 1.0


@pytest.mark.parametrize("gamma", [5.0, 1.0])
def test_min_snr_forms(gamma):
    ab = _bufs(1000)["alphas_cumprod"]
    assert OB.min_snr_weights(ab, gamma).numpy().tobytes() == OB.min_snr_weights(ab, gamma, "epsilon").numpy().tobytes()
    snr = ab.double() / (1.0 - ab.double())
    assert torch.equal(OB.min_snr_weights(ab, gamma), (torch.clamp(snr, max=gamma) / snr).float())          # the parent's expression
    for p in ("epsilon",) + PREDICTIONS:
        w = OB.min_snr_weights(ab, gamma, p)
        ref = min_snr64(ab, gamma, p)
        assert w.dtype == torch.float32 and torch.equal(w, ref.float())
    # the three are one weight on the x0-loss: w_eps SNR = w_v (SNR + 1) = w_x0
    we, wv, wx = (min_snr64(ab, gamma, p) for p in ("epsilon",) + PREDICTIONS)
    assert torch.allclose(we * snr, wx, rtol=1e-12, atol=0) and torch.allclose(wv * (snr + 1), wx, rtol=1e-12, atol=0)
    table = OB.loss_table("min_snr", gamma, ab, None, "v_prediction")
    assert np.array_equal(table, OB.min_snr_weights(ab, gamma, "v_prediction").numpy())
    assert np.array_equal(OB.loss_table("min_snr", gamma, ab, None), OB.min_snr_weights(ab, gamma).numpy())


def test_bad_values_raise_value_error():
    for bad in ("v", "eps", "x0", "V_PREDICTION", None, 1, ""):
        with pytest.raises(ValueError):
            OB.check_prediction_type(bad)
        with pytest.raises(ValueError):
            OB.min_snr_weights(_bufs()["alphas_cumprod"], 5.0, bad)
    for good in ("epsilon",) + PREDICTIONS:
        assert OB.check_prediction_type(good) == good
    ab = _bufs()["alphas_cumprod"]
    for fn in (ddim_step_table, ddim_x0_table):
        with pytest.raises(ValueError):
            fn(ab, ddim_timesteps(T, 10), 0.0, "velocity")
    conf = config(SM_H, T=10)
    conf["model"]["diffusion"]["prediction_type"] = "velocity"
    with pytest.raises(ValueError):
        BiologyAwareDiffusionModel(config=conf, **SM)
    conf["model"]["diffusion"]["prediction_type"] = "sample"
    assert BiologyAwareDiffusionModel(config=conf, **SM).prediction_type == "sample"
    assert BiologyAwareDiffusionModel(config=config(SM_H, T=10), **SM).prediction_type == "epsilon"


def _ckpt(pred):
    conf = config(SM_H, T=10)
    if pred is not None:
        conf["model"]["diffusion"]["prediction_type"] = pred
    return {"config": conf}


def test_checkpoint_type_against_config_type():
    assert checkpoint_prediction_type(_ckpt("v_prediction"), _ckpt(None)["config"]) == "v_prediction"
    assert checkpoint_prediction_type(_ckpt("sample"), {"model": {}}) == "sample"
    assert checkpoint_prediction_type(_ckpt(None), _ckpt(None)["config"]) is None            # a reference checkpoint: nothing to take over
    assert checkpoint_prediction_type({}, _ckpt(None)["config"]) is None
    assert checkpoint_prediction_type(_ckpt("v_prediction"), _ckpt("v_prediction")["config"]) is None
    assert checkpoint_prediction_type(_ckpt(None), _ckpt("epsilon")["config"]) is None
    for saved, asked in (("v_prediction", "epsilon"), ("v_prediction", "sample"), (None, "v_prediction"), ("sample", "v_prediction")):
        with pytest.raises(ValueError, match="prediction_type"):
            checkpoint_prediction_type(_ckpt(saved), _ckpt(asked)["config"])
    with pytest.raises(ValueError):
        checkpoint_prediction_type(_ckpt("velocity"), _ckpt(None)["config"])


def test_load_trained_model_adopts_or_rejects_the_checkpoints_type(tmp_path):
    """A tiny checkpoint built on the CPU: a config without the key adopts the checkpoint's type, a different one raises ValueError."""
    import pandas as pd
    conf = config(SM_H, T=10)
    conf["model"]["diffusion"]["prediction_type"] = "v_prediction"
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(config=conf, **SM)
    path = tmp_path / "ckpt.pt"
    torch.save({"epoch": 0, "model_state_dict": m.state_dict(), "val_loss": 0.0, "config": conf}, path)
    for fname, width in (("mutation_matrix_aligned.csv", SM["mutation_dim"]), ("expression_matrix_aligned.csv", SM["expression_dim"]),
                         ("pathway_scores.csv", SM["pathway_dim"])):
        pd.DataFrame(np.zeros((1, width)), index=["p0"]).to_csv(tmp_path / fname)
    load_conf = config(SM_H, T=10)
    load_conf["data"] = {"processed_dir": str(tmp_path)}
    got = load_trained_model(path, load_conf, "cpu")
    assert got.prediction_type == "v_prediction" and not got.training
    assert "prediction_type" not in load_conf["model"]["diffusion"]          # the caller's config is left alone
    load_conf["model"]["diffusion"]["prediction_type"] = "v_prediction"
    assert load_trained_model(path, load_conf, "cpu").prediction_type == "v_prediction"
    for other in ("epsilon", "sample"):
        load_conf["model"]["diffusion"]["prediction_type"] = other
        with pytest.raises(ValueError, match="prediction_type"):
            load_trained_model(path, load_conf, "cpu")


def test_abi_declares_the_prediction_entry_points():
    syms = L.exported_symbols()
    assert "osd_set_prediction" in syms and "osd_q_sample_target" in syms
    text = (ROOT / "include" / "osdiff.h").read_text()
    for name, value in (("OSD_PRED_EPSILON", "0"), ("OSD_PRED_V", "1"), ("OSD_PRED_SAMPLE", "2"), ("OSD_TP_TARGET", "(1 << 12)")):
        assert re.search(rf"#define\s+{name}\s+{re.escape(value)}(\s|$)", text), name
    assert (L.OSD_PRED_EPSILON, L.OSD_PRED_V, L.OSD_PRED_SAMPLE, L.OSD_TP_TARGET) == (0, 1, 2, 1 << 12)
    assert OB.PREDICTION_TYPES == {"epsilon": L.OSD_PRED_EPSILON, "v_prediction": L.OSD_PRED_V, "sample": L.OSD_PRED_SAMPLE}
    assert re.search(r"int\s+osd_set_prediction\s*\(\s*osd_handle\s*\*\s*h\s*,\s*int\s+type\s*\)", text)
    assert re.search(r"int\s+osd_q_sample_target\s*\(", text)
