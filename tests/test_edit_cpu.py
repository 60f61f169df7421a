"""CPU: the plans of an edit (ddim.edit_timesteps, ddim.ddim_inversion_table) and the definition of the noise map (osd_noise_map) in
float64 NumPy.  No GPU."""
import numpy as np
import pytest

from osteosarcoma_diffusionmodel_amd.ddim import (ddim_inversion_table, ddim_step_table, ddim_timesteps, edit_timesteps,
                                                  logsnr_timesteps)
from edit_helpers import noise_map_definition, replay, schedule


# ---- 1. edit_timesteps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S", [(100, 10), (1000, 50), (100, 100), (1000, 7)])
@pytest.mark.parametrize("strength", [0.04, 0.3, 0.6, 1.0])
@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
def test_edit_timesteps(T, S, strength, spacing):
    abar = schedule("cosine", T)[0]
    lv = edit_timesteps(T, S, strength, abar, spacing)
    K = max(1, int(round(strength * S)))
    plan = ddim_timesteps(T, S) if spacing == "uniform" else logsnr_timesteps(abar, S)
    assert lv.dtype == np.int32 and lv[0] == 0 and (np.diff(lv) > 0).all()
    assert lv.size in (K, K + 1)
    assert np.array_equal(lv[lv.size - K:], plan[:K]) or (plan[0] == 0 and np.array_equal(lv, plan[:K]))
    if strength == 1.0:
        assert np.array_equal(lv[-S:], plan) and lv.size == S + (plan[0] != 0)


def test_edit_timesteps_rejects():
    for kw in (dict(strength=0.0), dict(strength=-0.1), dict(strength=1.01), dict(strength=float("nan")), dict(strength=0.5, spacing="cosine"),
               dict(strength=0.5, spacing="logsnr"), dict(strength=0.5, S=0), dict(strength=0.5, S=101)):
        args = dict(T=100, S=10)
        args.update(kw)
        with pytest.raises(ValueError):
            edit_timesteps(**args)
    with pytest.raises(ValueError):
        edit_timesteps(100, 10, 0.5, schedule("cosine", 50)[0], "logsnr")      # a schedule of another length


# ---- 2. the inversion table against the decode table -----------------------------------------------------------------------
def _ulps(x, k=4):
    return k * float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("T", [100, 1000])
@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction", "sample"])
def test_inversion_table_undoes_the_decode_row(prediction, kind, T):
    """With the network output held consistent across an adjacent pair of levels, the eta = 0 decode row (A_d, B_d) undoes the inversion
    row (A_i, B_i): x = A_d (A_i x + B_i out) + B_d out'.  An epsilon and a sample model keep a constant output consistent (out' = out:
    the same eps, the same x0), so A_d A_i = 1 and A_d B_i + B_d = 0.  A v-model's output turns with the level -- v = a eps - b x0 --, so
    a constant v is NOT the same (x0, eps) at both levels and those two products are cos^2 of the angle between the levels, not 1; the
    consistent output is the one that reads as the same x0^ at the upper level, out' = (a' x' - x0^) / b' with x0^ = a x - b out, which
    gives the same two identities with one more term each.  Each table is rounded once from float64, so a term with two rounded
    factors is off by at most one fp32 ulp: 4 ulps of the largest term bound the sums."""
    abar, sa, s1 = schedule(kind, T)
    sched = dict(sqrt_alphas_cumprod=sa, sqrt_one_minus_alphas_cumprod=s1)
    for levels in (edit_timesteps(T, 10, 1.0), edit_timesteps(T, min(T, 50), 0.5, abar, "logsnr"), np.arange(0, 12, dtype=np.int32)):
        tau_d, dec = ddim_step_table(abar, levels, 0.0, prediction, **sched)
        tau_i, inv = ddim_inversion_table(abar, levels, prediction, **sched)
        n = levels.size - 1
        assert inv.dtype == np.float32 and inv.shape == (n, 4) and tau_i.dtype == np.int32
        assert np.array_equal(tau_i, levels[:-1][::-1]) and (inv[:, 2:] == 0).all()      # the chain's order; C = 0 in every row, row 0 included
        for j in range(n):
            Ai, Bi = (float(v) for v in inv[n - 1 - j, :2])
            Ad, Bd = (float(v) for v in dec[j + 1, :2])
            assert tau_i[n - 1 - j] == levels[j] and tau_d[j + 1] == levels[j + 1]
            if prediction == "v_prediction":
                P, Q = float(sa[levels[j]]), -float(s1[levels[j]])
                an, bn = float(sa[levels[j + 1]]), float(s1[levels[j + 1]])
                cx = [Ad * Ai, Bd * an * Ai / bn, -Bd * P / bn]
                co = [Ad * Bi, Bd * an * Bi / bn, -Bd * Q / bn]
            else:
                cx, co = [Ad * Ai], [Ad * Bi, Bd]
            assert abs(sum(cx) - 1.0) <= _ulps(max(1.0, *map(abs, cx))), (prediction, kind, T, j, cx)
            assert abs(sum(co)) <= _ulps(max(map(abs, co))), (prediction, kind, T, j, co)


def test_inversion_table_rejects():
    abar = schedule("cosine", 100)[0]
    for levels in ([0], [5, 5, 9], [9, 5], [-1, 4], [0, 100]):
        with pytest.raises(ValueError):
            ddim_inversion_table(abar, levels)
    with pytest.raises(ValueError):
        ddim_inversion_table(abar, [0, 9], "velocity")
    one = abar.copy()
    one[0] = 1.0
    with pytest.raises(ValueError, match="b = 0"):
        ddim_inversion_table(one, [0, 9])


# ---- 3. the definition of the noise map ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction", "sample"])
def test_noise_map_definition_round_trip(prediction):
    """float64 NumPy, a toy affine denoiser: replaying A y + B out + C z from x_start reproduces every y_{s-1}, and the last step returns
    A_0 y_0 + B_0 out_0."""
    T, n, D = 100, 7, 13
    abar, sa, s1 = schedule("cosine", T)
    levels = edit_timesteps(T, 10, 0.8)
    taus, coef = ddim_step_table(abar, levels, 1.0, prediction, sqrt_alphas_cumprod=sa, sqrt_one_minus_alphas_cumprod=s1)
    coef = coef.astype(np.float64)
    assert coef[0, 2] == 0 and (coef[1:, 2] > 0).all()
    rng = np.random.default_rng(3)
    W, c = rng.standard_normal((D, D)) / np.sqrt(D), rng.standard_normal(D)
    x0, eps = rng.standard_normal((n, D)), rng.standard_normal((levels.size, n, D))

    def denoiser(y, s):
        return y @ W * (0.5 + taus[s] / T) + c

    y, cz, outs = noise_map_definition(x0, eps, sa.astype(np.float64), s1.astype(np.float64), taus, coef, denoiser)
    states = replay(y[-1], cz, coef, denoiser)
    for s in range(1, levels.size):
        assert np.abs(states[s] - y[s - 1]).max() <= 1e-12, s
    assert np.abs(states[0] - (coef[0, 0] * y[0] + coef[0, 1] * outs[0])).max() <= 1e-12
    # the draws are what the chain adds divided by C: finite, and not the injected eps
    z = [cz[levels.size - 1 - s] / coef[s, 2] for s in range(1, levels.size)]
    assert all(np.isfinite(v).all() for v in z)
