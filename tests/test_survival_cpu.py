"""CPU: the survival utility's host code (osteosarcoma_diffusionmodel_amd/survival.py), the float64 restatement the GPU tests
measure the kernels against (tests/survival_helpers.py), and the argument checks of the three C entry points, which happen on the
host before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import survival as SV
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, survival_metrics
from survival_helpers import (SurvivalNumpyKernels, concordance_loop, cox_brute64, cox_case, cox_eval64, cox_eval_fn,
                              penalised_cox_gradient64, planted_survival)


# ---- 1. the scan form is the risk-set form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,ties", [(257, 130, "distinct"), (257, 130, "grid"), (257, 130, "equal"), (1, 5, "grid")])
def test_scan_form_equals_the_risk_set_sums(rows, D, ties):
    x, c, s, w, time, event = cox_case(rows, D, ties)
    if rows == 1:
        event = np.ones(1)
    ref = cox_eval64(x, c, s, w, time, event)
    loss, grad = cox_brute64(x, c, s, w, time, event)
    assert (np.unique(time).size == rows) == (ties == "distinct" or rows == 1) and (np.unique(time).size == 1) == (ties == "equal" or rows == 1)
    el = abs(ref["loss"] - loss) / max(ref["loss_scale"], 1e-300) if ref["loss_scale"] > 0 else abs(ref["loss"] - loss)
    eg = np.max(np.abs(ref["grad"] - grad) / np.maximum(ref["grad_scale"], 1e-300)) if ref["grad_scale"].max() > 0 else np.abs(ref["grad"] - grad).max()
    print(f"{rows}x{D} {ties}: loss {el:.3e}, gradient {eg:.3e}")
    assert el <= 1e-13 and eg <= 1e-12


def test_all_censored_is_exactly_zero():
    x, c, s, w, time, _ = cox_case(257, 130, "censored")
    ref = cox_eval64(x, c, s, w, time, np.zeros(257))
    assert ref["loss"] == 0.0 and not ref["grad"].any() and not ref["resid"].any()


def test_a_single_event_row_is_exactly_zero():
    x, c, s, w, time, _ = cox_case(1, 5, "grid")
    ref = cox_eval64(x, c, s, w, time, np.ones(1))
    assert ref["loss"] == 0.0 and not ref["grad"].any()
    loss, grad = cox_brute64(x, c, s, w, time, np.ones(1))
    assert loss == 0.0 and not grad.any()


# ---- 2. concordance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 60, 301])
def test_concordance_counts_equal_the_double_loop(n):
    rs = np.random.default_rng(n)
    time = 30.0 * rs.integers(1, 6, n)                            # few distinct times and risks: ties everywhere
    event = (rs.random(n) < 0.6).astype(np.float64)
    risk = rs.integers(-2, 3, n).astype(np.float64) / 4
    want = concordance_loop(time, event, risk)
    assert SV.concordance_counts(time, event, risk) == want
    assert SV.concordance_counts(time, event, risk, chunk=3) == want
    assert want[0] == want[1] + want[2] + want[3]
    if want[0]:
        assert SV.concordance_index(time, event, risk) == (want[1] + 0.5 * want[3]) / want[0]
    else:
        with pytest.raises(ValueError, match="comparable"):
            SV.concordance_index(time, event, risk)


def test_concordance_of_a_perfect_and_a_reversed_risk():
    time = np.array([5.0, 1.0, 3.0, 2.0, 4.0])
    event = np.array([1.0, 1.0, 0.0, 1.0, 1.0])
    assert SV.concordance_index(time, event, -time) == 1.0 and SV.concordance_index(time, event, time) == 0.0
    assert SV.concordance_index(time, event, np.zeros(5)) == 0.5
    assert SV.concordance_counts(time, event, -time)[0] == 4 + 3 + 1      # the event at 1 has 4 later partners, at 2: 3 (a censored partner counts), at 4: 1, at 5: none
    for bad in ((np.array([1.0, np.nan]), np.ones(2), np.ones(2)), (np.ones(2), np.array([0.0, 2.0]), np.ones(2)), (np.ones(2), np.ones(3), np.ones(2))):
        with pytest.raises(ValueError):
            SV.concordance_counts(*bad)


# ---- 3. the driver --------------------------------------------------------------------------------------------------------------------
def test_fit_cox_reaches_tol_on_the_float64_objective():
    x, c, s, _, time, event = cox_case(257, 130, "grid")
    n, l2, tol = 257.0, 1e-2, 1e-5
    fit = SV.fit_cox(cox_eval_fn(x, c, s, time, event), 130, n, l2, tol=tol)
    g = penalised_cox_gradient64(x, c, s, fit["w"], time, event, n, l2)
    print(f"fit_cox: {fit['iterations']} iterations, |g|_inf {np.abs(g).max():.3e}")
    assert fit["converged"] and fit["iterations"] >= 5 and np.abs(g).max() <= tol and fit["grad_inf_norm"] == np.abs(g).max()
    for bad in (dict(D=0, n=n, l2=l2), dict(D=130, n=0.0, l2=l2), dict(D=130, n=n, l2=-1.0)):
        with pytest.raises(ValueError):
            SV.fit_cox(cox_eval_fn(x, c, s, time, event), **bad)


def test_fit_cox_rejects_a_non_finite_step():
    """An eval_fn that reports an emptied risk set (a non-finite loss) beyond |w| = 1 never gets there."""
    x, c, s, _, time, event = cox_case(33, 6, "grid")
    inner = cox_eval_fn(x, c, s, time, event)
    def fn(w):
        loss, g = inner(w)
        return (float("inf") if np.abs(w).max() > 1.0 else loss), g
    fit = SV.fit_cox(fn, 6, 33.0, 1e-2)
    assert np.isfinite(fit["w"]).all() and np.abs(fit["w"]).max() <= 1.0


# ---- 4. the C entry points check their arguments on the host --------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments_without_a_device():
    lib = L.lib()
    t, d = np.array([3.0, 1.0, 2.0]), np.array([1.0, 0.0, 1.0])
    plan = C.c_void_p()
    create = lambda time, event, rows, out=plan: lib.osd_val_cox_plan_create(0, None, time.ctypes.data if time is not None else None,
                                                                             event.ctypes.data if event is not None else None, rows,
                                                                             C.byref(out) if out is not None else None)
    assert create(t, d, 0) == L.OSD_EINVAL and create(t, d, -1) == L.OSD_EINVAL and create(t, d, 2 ** 31) == L.OSD_EINVAL
    assert create(None, d, 3) == L.OSD_EINVAL and create(t, None, 3) == L.OSD_EINVAL and create(t, d, 3, None) == L.OSD_EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert create(np.array([3.0, bad, 2.0]), d, 3) == L.OSD_EINVAL and b"finite" in lib.osd_last_error()
    for bad in (2.0, -1.0, 0.5, np.nan):
        assert create(t, np.array([1.0, bad, 0.0]), 3) == L.OSD_EINVAL and b"flag" in lib.osd_last_error()
    assert plan.value is None
    assert lib.osd_val_cox_plan_destroy(None) == L.OSD_OK
    loss = C.c_double()
    assert lib.osd_val_cox_eval(None, None, 3, 4, 4, None, None, None, C.byref(loss), None, None) == L.OSD_EINVAL
    counts = (C.c_int64 * 4)()
    x = torch.zeros(4)
    for n in (0, -1, 2 ** 31):
        assert lib.osd_val_concordance(None, 0, L.ptr(x), L.ptr(x), L.ptr(x), n, counts) == L.OSD_EINVAL
    assert lib.osd_val_concordance(None, 0, None, L.ptr(x), L.ptr(x), 4, counts) == L.OSD_EINVAL
    assert lib.osd_val_concordance(None, 0, L.ptr(x), L.ptr(x), L.ptr(x), 4, None) == L.OSD_EINVAL
    assert lib.osd_val_concordance(None, -1, L.ptr(x), L.ptr(x), L.ptr(x), 4, counts) == L.OSD_EINVAL


# ---- 5. end to end on the stand-in kernels ------------------------------------------------------------------------------------------
def _pipeline(permute):
    (train, train_s), (synth, synth_s), (test, test_s) = planted_survival(600, 130, 3), planted_survival(600, 130, 7), planted_survival(300, 130, 11)
    if permute:
        synth_s = synth_s[np.random.default_rng(0).permutation(len(synth_s))]
    t = lambda a: torch.from_numpy(np.array(a))
    return survival_metrics(SurvivalNumpyKernels(), t(train), train_s, t(synth), synth_s, t(test), test_s, l2=1e-2, return_fits=True)


def test_planted_hazards_are_recovered_and_permuted_ones_are_not():
    out, fits = _pipeline(False)
    bad, _ = _pipeline(True)
    print(out, [(f["iterations"], f["converged"]) for f in fits], bad["survival_tstr_cindex"])
    assert set(out) == {"survival_tstr_cindex", "survival_trtr_cindex", "survival_cindex_gap", "survival_coef_cosine",
                        "survival_comparable_pairs", "survival_event_share_real_train", "survival_event_share_synthetic",
                        "survival_event_share_real_test"}
    assert all(f["converged"] for f in fits)
    assert out["survival_trtr_cindex"] >= 0.70 and out["survival_tstr_cindex"] >= 0.70
    assert abs(out["survival_cindex_gap"]) <= 0.05 and out["survival_cindex_gap"] == out["survival_trtr_cindex"] - out["survival_tstr_cindex"]
    assert 0.40 <= bad["survival_tstr_cindex"] <= 0.60
    assert bad["survival_trtr_cindex"] == out["survival_trtr_cindex"]      # trained on the same real rows
    assert out["survival_coef_cosine"] > 0.5 > bad["survival_coef_cosine"]
    assert 0.3 < out["survival_event_share_real_test"] < 0.9 and out["survival_comparable_pairs"] > 1000


def test_cohort_errors_name_the_cohort():
    (train, train_s), (test, test_s) = planted_survival(60, 8, 3), planted_survival(40, 8, 11)
    t = lambda a: torch.from_numpy(np.array(a))
    k = SurvivalNumpyKernels()
    censored = train_s.copy()
    censored[:, 1] = 0.0
    with pytest.raises(ValueError, match="synthetic cohort has no event"):
        survival_metrics(k, t(train), train_s, t(train), censored, t(test), test_s)
    with pytest.raises(ValueError, match="real_train cohort has no event"):
        survival_metrics(k, t(train), censored, t(train), train_s, t(test), test_s)
    late = test_s.copy()
    late[:, 1] = 0.0
    late[np.argmax(late[:, 0]), 1] = 1.0                          # the only event is the last time: nothing comes later
    with pytest.raises(ValueError, match="real_test cohort has no comparable pair"):
        survival_metrics(k, t(train), train_s, t(train), train_s, t(test), late)
    half = train_s.copy()
    half[0, 1] = 0.5
    with pytest.raises(ValueError, match="flags of synthetic"):
        survival_metrics(k, t(train), train_s, t(train), half, t(test), test_s)


def test_validator_argument_errors_need_no_device():
    x, s = planted_survival(60, 8, 3)
    sharded = BiologicalValidator({"evaluation": {}}, device="cuda:0", sharded=True)
    with pytest.raises(NotImplementedError, match="sharded.*risk set"):
        sharded.survival_utility(x, s, x, s, x, s)
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.survival_utility(x, s, x[:, :3], s, x, s)            # said first, whatever the arguments
