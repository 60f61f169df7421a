"""CPU: the host code of the univariate Cox screen (survival.univariate_cox, survival.cox_screen, validation.prognostic_metrics), the
float64 restatement the GPU tests measure the kernel against (tests/prognostic_helpers.py), and what osd_val_cox_score promises
without a device: its declaration, its binding and the argument checks that come before any device call."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import survival as SV
from osteosarcoma_diffusionmodel_amd.validation import COXS_ROWS, BiologicalValidator, prognostic_metrics
from prognostic_helpers import (PrognosticNumpyKernels, cox_score64, cox_score_brute64, logrank_chi2, score_eval_fn)
from survival_helpers import cox_case, cox_eval64, planted_survival

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("loglik", "score", "info")


def _beta(D, seed=0):
    return np.random.default_rng(1009 * D + seed).uniform(-1.0, 1.0, D)


# ---- 1. the scan form is the risk-set form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("rows,D,ties", [(257, 130, "distinct"), (257, 130, "grid"), (257, 130, "equal"), (257, 130, "events"),
                                         (33, 6, "grid"), (1, 5, "grid")])
def test_scan_form_equals_the_risk_set_sums(rows, D, ties, with_beta):
    x, c, s, _, time, event = cox_case(rows, D, ties)
    if rows == 1:
        event = np.ones(1)
    s = s.copy()
    s[1] = 0.0                                                    # a dropped column
    beta = _beta(D) if with_beta else None
    bound = cox_score64(x, c, s, time, event)["absmax"] if with_beta else None
    ref = cox_score64(x, c, s, time, event, beta, bound)
    brute = cox_score_brute64(x, c, s, time, event, beta, bound)
    for name, b in zip(FIELDS, brute):
        scale = ref[name + "_scale"]
        live = scale > 0
        assert not ref[name][~live].any() and not b[~live].any()
        err = float(np.max(np.abs(ref[name] - b)[live] / scale[live])) if live.any() else 0.0
        print(f"{rows}x{D} {ties} beta={with_beta} {name}: {err:.3e}")
        assert err <= 1e-12
    assert not ref["loglik"][1] and not ref["score"][1] and not ref["info"][1] and not ref["absmax"][1]
    if with_beta:
        assert ref["max_arg"] <= 2.0 * np.abs(beta * bound).max() and (ref["info"] >= -1e-12 * ref["info_scale"]).all()


def test_all_censored_is_exactly_zero():
    x, c, s, _, time, event = cox_case(257, 130, "censored")
    for beta in (None, _beta(130)):
        ref = cox_score64(x, c, s, time, event, beta, None if beta is None else np.full(130, 10.0))
        assert not any(ref[name].any() for name in FIELDS) and ref["absmax"].all()


# ---- 2. the score test of a 0/1 covariate is the log-rank test ------------------------------------------------------------------------
@pytest.mark.parametrize("rows,seed", [(40, 0), (200, 1), (257, 2)])
def test_z_squared_is_the_logrank_chi_square(rows, seed):
    rs = np.random.default_rng(seed)
    time = rs.permutation(rows).astype(np.float64) + 1.0          # distinct
    event = (rs.random(rows) < 0.6).astype(np.float64)
    group = (rs.random(rows) < 0.4).astype(np.float32)
    for center, scale in ((0.0, 1.0), (0.4, 2.5)):                 # the statistic does not see the standardisation
        r = cox_score64(group[:, None], [center], [scale], time, event)
        z2 = float(r["score"][0] ** 2 / r["info"][0])
        want = logrank_chi2(group, time, event)
        print(f"rows {rows}: z^2 {z2!r}, log-rank {want!r}")
        assert abs(z2 - want) <= 1e-10 * want


# ---- 3. at beta = 0 the score is minus the gradient of the multivariate likelihood at w = 0 ------------------------------------------
@pytest.mark.parametrize("rows,D,ties", [(257, 130, "grid"), (257, 130, "distinct"), (33, 6, "grid")])
def test_score_at_zero_is_minus_cox_eval_gradient(rows, D, ties):
    x, c, s, _, time, event = cox_case(rows, D, ties)
    ref = cox_eval64(x, c, s, np.zeros(D), time, event)
    got = cox_score64(x, c, s, time, event)
    err = float(np.max(np.abs(got["score"] + ref["grad"]) / ref["grad_scale"]))
    print(f"{rows}x{D} {ties}: {err:.3e}")
    assert err <= 1e-12


# ---- 4. the driver ------------------------------------------------------------------------------------------------------------------
def _driver_case():
    x, surv = planted_survival(600, 130, 3)
    x = np.array(x[:, :6])
    time, event = surv[:, 0] + 1e-3 * np.arange(600), surv[:, 1]      # distinct: a tie would break the separation
    rank = np.argsort(np.argsort(-time, kind="stable"), kind="stable").astype(np.float32)
    x[:, 4] = rank / 600.0                                        # the later the position in descending time, the larger: separates perfectly
    x[:, 5] = 1.0                                                 # constant
    center = x.astype(np.float64).mean(0).astype(np.float32)
    scale = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0], dtype=np.float32)
    return x, center, scale, time, np.ones_like(event), event


def test_univariate_cox_matches_a_scalar_optimiser():
    from scipy.optimize import minimize_scalar
    x, center, scale, time, _, event = _driver_case()
    bound = cox_score64(x, center, scale, time, event)["absmax"]
    fit = SV.univariate_cox(score_eval_fn(x, center, scale, time, event, bound), 6, bound)
    print({k: v[:4] for k, v in fit.items()})
    for col in range(3):
        def neg(b, col=col):
            beta = np.zeros(6)
            beta[col] = b
            return -cox_score64(x, center, scale, time, event, beta, bound)["loglik"][col]
        best = minimize_scalar(neg, bracket=(-1.0, 1.0), tol=1e-12).x
        assert fit["converged"][col] and abs(fit["beta"][col] - best) <= 1e-6 and 1 <= fit["iterations"][col] <= 15
    z = fit["z_wald"][:4]
    assert np.allclose(z, fit["beta"][:4] / fit["se"][:4]) and (fit["p_wald"][:4] < 1e-3).all()
    assert np.array_equal(np.sign(fit["beta"][:4]), [1.0, -1.0, 1.0, -1.0])


def test_a_separating_column_ends_at_the_clamp_and_a_dead_one_fails():
    x, center, scale, time, all_events, _ = _driver_case()
    bound = cox_score64(x, center, scale, time, all_events)["absmax"]
    fit = SV.univariate_cox(score_eval_fn(x, center, scale, time, all_events, bound), 6, bound, max_abs_eta=30.0)
    assert not fit["converged"][4] and not fit["failed"][4] and np.isfinite(fit["beta"][4])
    assert abs(abs(fit["beta"][4]) * bound[4] - 30.0) <= 1e-9      # at the clamp
    assert fit["failed"][5] and not fit["converged"][5] and np.isnan(fit["beta"][5]) and np.isnan(fit["se"][5])
    k = PrognosticNumpyKernels()
    with k.cox_plan(time, all_events) as plan:
        for mle in (True, False):
            scr = SV.cox_screen(k, torch.from_numpy(x), plan, center, scale, mle=mle)
            assert np.isnan(scr["q"][5]) and np.isnan(scr["effect"][5]) and scr["failed"][5] and np.isfinite(scr["q"][:5]).all()
            from osteosarcoma_diffusionmodel_amd.diffexp import bh_qvalues
            assert np.array_equal(scr["q"][:5], bh_qvalues(scr["p_score"][:5]))      # the dead column is not among the tests
            assert np.array_equal(scr["hr"][:5], np.exp(scr["effect"][:5]))
    with pytest.raises(ValueError):
        SV.univariate_cox(lambda b: (b, b, b), 0, [])


# ---- 5. planted cohorts, end to end on the stand-in kernels ----------------------------------------------------------------------------
def _planted(permute, **kw):
    (real, real_s), (synth, synth_s) = planted_survival(600, 130, 3), planted_survival(600, 130, 7)
    if permute:
        synth_s = synth_s[np.random.default_rng(0).permutation(len(synth_s))]
    t = lambda a: torch.from_numpy(np.array(a))
    return prognostic_metrics(PrognosticNumpyKernels(), t(real), real_s, t(synth), synth_s, **kw)


def test_planted_prognostic_features_are_found_and_permuted_ones_are_not():
    out, rows = _planted(False)
    bad, bad_rows = _planted(True)
    hits = lambda scr: set(np.nonzero(scr["q"] < 0.05)[0].tolist())
    print(out, rows["real"]["effect"][:4], bad)
    assert hits(rows["real"]) == {0, 1, 2, 3} and hits(rows["synthetic"]) == {0, 1, 2, 3}
    assert np.abs(rows["real"]["effect"][:4] - np.array([0.58, -0.64, 0.30, -0.30])).max() <= 0.01
    assert out["prog_real_hits"] == 4 and out["prog_synth_hits"] == 4 and out["prog_precision"] == 1.0 and out["prog_recall"] == 1.0
    assert out["prog_sign_agreement"] == 1.0
    assert hits(bad_rows["synthetic"]) == set() and bad["prog_recall"] == 0.0 and bad["prog_synth_hits"] == 0
    assert abs(bad["prog_effect_slope"]) < 0.05
    assert hits(bad_rows["real"]) == {0, 1, 2, 3}                 # the real screen does not see the synthetic cohort
    from osteosarcoma_diffusionmodel_amd.diffexp import contrast_summary
    keys = {f"prog_{key}" for key in contrast_summary({"effect": np.zeros(2), "q": np.ones(2)}, {"effect": np.zeros(2), "q": np.ones(2)})}
    assert set(out) == keys | {"prog_features", "prog_constant_features", "prog_not_converged_real", "prog_not_converged_synth",
                               "prog_events_real", "prog_events_synth", "prog_max_abs_z_real", "prog_max_abs_z_synth"}
    assert out["prog_features"] == 130 and out["prog_constant_features"] == 0
    assert out["prog_not_converged_real"] == 0 and out["prog_not_converged_synth"] == 0
    assert out["prog_events_real"] == int(planted_survival(600, 130, 3)[1][:, 1].sum()) and out["prog_max_abs_z_real"] > 5


def test_one_step_effects_find_the_same_features():
    out, rows = _planted(False, mle=False)
    assert out["prog_precision"] == 1.0 and out["prog_recall"] == 1.0 and out["prog_real_hits"] == 4
    scr = rows["real"]
    assert np.array_equal(scr["effect"], scr["score0"] / scr["info0"])


def test_a_constant_real_column_is_left_out_and_counted_and_blocks_follow():
    (real, real_s), (synth, synth_s) = planted_survival(200, 12, 3), planted_survival(220, 12, 7)
    real, synth = np.array(real), np.array(synth)
    real[:, 5] = 2.0
    synth[:, 7] = -1.0                                            # constant in the synthetic cohort only: no signal there
    t = torch.from_numpy
    out, rows = prognostic_metrics(PrognosticNumpyKernels(), t(real), real_s, t(synth), synth_s, bounds=[0, 4, 12],
                                   block_names=["a", "b"])
    assert out["prog_features"] == 11 and out["prog_constant_features"] == 1 and not rows["live"][5] and rows["scale"][5] == 0
    assert out["prog_not_converged_synth"] == 1 and out["prog_not_converged_real"] == 0
    assert np.isnan(rows["real"]["q"][5]) and np.isnan(rows["synthetic"]["effect"][7])
    assert "prog_effect_pearson_a" in out and "prog_effect_pearson_b" in out and np.isfinite(out["prog_effect_pearson"])
    assert out["prog_max_gap_feature"] != 5


def test_cohort_errors_name_the_cohort():
    (real, real_s), (synth, synth_s) = planted_survival(60, 8, 3), planted_survival(50, 8, 7)
    t = lambda a: torch.from_numpy(np.array(a))
    k = PrognosticNumpyKernels()
    censored = synth_s.copy()
    censored[:, 1] = 0.0
    with pytest.raises(ValueError, match="synthetic cohort has no event"):
        prognostic_metrics(k, t(real), real_s, t(synth), censored)
    censored = real_s.copy()
    censored[:, 1] = 0.0
    with pytest.raises(ValueError, match="real cohort has no event"):
        prognostic_metrics(k, t(real), censored, t(synth), synth_s)
    with pytest.raises(ValueError, match="survival matrix of synthetic"):
        prognostic_metrics(k, t(real), real_s, t(synth), synth_s[:10])
    half = real_s.copy()
    half[0, 1] = 0.5
    with pytest.raises(ValueError, match="flags"):
        prognostic_metrics(k, t(real), half, t(synth), synth_s)


def test_sharded_validator_raises_without_a_device():
    x, s = planted_survival(60, 8, 3)
    sharded = BiologicalValidator({"evaluation": {}}, device="cuda:0", sharded=True)
    with pytest.raises(ValueError, match="sharded.*risk set"):
        sharded.prognostic_fidelity(x, s, x, s)


# ---- 6. the C entry point: declared, bound, and it checks its arguments on the host ----------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_point():
    text = (ROOT / "include" / "osdiff.h").read_text()
    assert re.search(r"\bint\s+osd_val_cox_score\s*\(", text)
    assert int(re.search(r"#define\s+OSD_COXS_ROWS\s+(\d+)", text).group(1)) == L.OSD_COXS_ROWS == COXS_ROWS
    assert "osd_val_cox_score" in L.exported_symbols() and hasattr(L.lib(), "osd_val_cox_score")


def test_c_entry_point_refuses_bad_arguments_without_a_device():
    lib = L.lib()
    x = torch.zeros(16)
    o = torch.zeros(4, dtype=torch.float64)
    p = L.ptr
    fake = C.c_void_p(1)                                          # never followed: every call below fails a check that comes first
    call = lib.osd_val_cox_score
    assert call(None, p(x), 3, 4, 4, p(x), p(x), None, None, p(o), p(o), p(o), None) == L.OSD_EINVAL      # no plan
    assert call(fake, None, 3, 4, 4, p(x), p(x), None, None, p(o), p(o), p(o), None) == L.OSD_EINVAL      # no X
    assert call(fake, p(x), 0, 4, 4, p(x), p(x), None, None, p(o), p(o), p(o), None) == L.OSD_EINVAL      # rows
    assert call(fake, p(x), 3, 4, 0, p(x), p(x), None, None, p(o), p(o), p(o), None) == L.OSD_EINVAL      # D = 0
    assert call(fake, p(x), 3, 8193, 8193, p(x), p(x), None, None, p(o), p(o), p(o), None) == L.OSD_EINVAL
    assert call(fake, p(x), 3, 3, 4, p(x), p(x), None, None, p(o), p(o), p(o), None) == L.OSD_EINVAL      # ld < D
    for hole in range(3):
        outs = [p(o), p(o), p(o)]
        outs[hole] = None
        assert call(fake, p(x), 3, 4, 4, p(x), p(x), None, None, *outs, None) == L.OSD_EINVAL
    assert b"bad argument" in lib.osd_last_error()
