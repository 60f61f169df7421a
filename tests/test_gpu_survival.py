"""GPU: the Cox partial-likelihood kernels (osd_val_cox_eval: cox_eta_kernel, the scans, cox_grad_kernel + cox_reduce, csrc/cox.hip),
the concordance kernel beside them, and ``BiologicalValidator.survival_utility`` above them, against the float64 restatement of
tests/survival_helpers.py evaluated on the same fp32 inputs.

Shapes (rows, D): (1, 5), (33, 6), (257, 130), (515, 5142), (100001, 8) -- one row; row tails; D below one 16-byte vector per lane;
D % 4 == 2; the reference's width (three column quads per lane, seven waves); and (100001, 8), whose 758 items of 132 rows have MORE
THAN ONE fp32 RUN AND A RAGGED LAST ONE (a run of OSD_GLM_RUN_ROWS = 128 rows, then one of 4; a last item of 77 rows) and whose
scans span 98 blocks of 1024 positions.  Every shape in the three layouts of test_gpu_utility.py (dense, aligned slice, unaligned
slice) on a 30-day grid of times; (257, 130) also with distinct times, all times equal, all censored (exact zeros) and all events;
(100001, 8) also with only 50 distinct times, so that every scan-block boundary falls inside a tie group.

  * scores, loss and gradient against float64, each error normalised by its natural scale (sum |w u| per score; sum delta |eta - m -
    log S|; sum |r u| per column); where that scale is 0 (all censored, a single row) the device must give the reference's exact 0.

    Measured, the largest over the cases: scores 1.630e-7 (100001 x 8, whose few small weights cancel), gradient 1.347e-7 and loss
    3.542e-8 (both at 33 x 6); at 515 x 5142 1.1e-8, 9.0e-8 and 2.2e-9; at 257 x 130 with distinct times / one time / all events the
    gradient 5.6e-8 / 4.3e-8 / 6.9e-8; at 100001 x 8 with 50 distinct times 1.6e-7, 1.8e-8 and 7.5e-10.  Asserted: 4 x that.
    It may not exceed what the rounding model allows: the scores are osd_val_glm_eval's (same arithmetic, SCORE_CEILING =
    34 x 2^-24 of test_gpu_utility.py); a gradient entry has one rounding for the residual (double ->
    fp32), one per centred value, per product and per accumulate within a run, double above: (OSD_GLM_RUN_ROWS + 9) x 2^-24, plus
    what the scores' error does to the residual through exp: with |d eta| <= SCORE_CEILING x max S (S the score's own scale),
    |d r_j| <= 2 e_j c_j max |d eta| (the row's own e and every risk-set share 1 / S_i sum_k e_k d eta_k move by at most that), so
    kappa_g = max_c 2 max S sum_j e_j c_j |u_jc| / sum_j |r_j u_jc|; the loss is summed in double, |d loss| <= 2 (events) max |d eta|,
    kappa_l = 2 max S (events) / sum delta |eta - m - log S|.  Both factors come from the float64 reference of the tested data; over
    the cases the ceilings come to 1.9e-4 (gradient) and 3.6e-5 (loss).
  * at w = 0 every e is 1, the scans add integers, and the loss is -sum delta log S: relative error <= 1e-13 against numpy
    (measured: 1.6e-16, 1.7e-16 and 0).
  * concordance: the four int64 counts EQUAL the host's.
  * the fit: the float64 gradient of the penalised objective at the w the device fit returns; measured at 257 x 130, l2 = 1e-2:
    |g|_inf = 1.704e-5 after the 200 iterations max_iter allows (the device's own gradient says 1.702e-5) -- above the default tol of 1e-5, as the GLM fit's:
    the fit ends at the noise floor of an objective whose scores are fp32, and reports converged=False.  Asserted: 4 x that.
  * end to end: |d C-index| between the validator and the float64 pipeline (same driver, float64 kernels) on the planted cohorts;
    measured: 0 -- the two pipelines order the 300 test patients identically, faithful and permuted cohort alike, so all 31 920
    comparable pairs count the same (one pair moved would be 1.6e-5); the coefficient cosines differ by 1.6e-8.  Asserted: 4 x that,
    which is equality."""
import functools

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import survival as SV
from osteosarcoma_diffusionmodel_amd.validation import (CONC_I_TILE, CONC_J_CHUNK, GLM_RUN_ROWS, BiologicalValidator, DeviceKernels,
                                                        survival_metrics)
from survival_helpers import (SurvivalNumpyKernels, cox_case, cox_eval64, penalised_cox_gradient64, planted_survival)
from utility_helpers import SQUARED

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5), (33, 6), (257, 130), (515, 5142), (100001, 8)]
LAYOUTS = ["dense", "slice_aligned", "slice_unaligned"]
CASES = ([(rows, D, "grid", layout) for rows, D in SHAPES for layout in LAYOUTS] +
         [(257, 130, ties, "dense") for ties in ("distinct", "equal", "censored", "events")] + [(100001, 8, "fifty", "dense")])
EPS = 2.0 ** -24
SCORE_OBSERVED, GRAD_OBSERVED, LOSS_OBSERVED = 1.630e-7, 1.347e-7, 3.542e-8      # measured maxima over CASES
SCORE_TOL, GRAD_TOL, LOSS_TOL = 4 * SCORE_OBSERVED, 4 * GRAD_OBSERVED, 4 * LOSS_OBSERVED
SCORE_CEILING = 34 * EPS          # test_gpu_utility.py: the GLM's
FIT_OBSERVED = 1.704e-5           # measured |float64 penalised gradient|_inf at the device fit's w
E2E_OBSERVED = 0.0                # measured max |d C-index| of the validator against the float64 pipeline: the same pair counts
CONF = {"evaluation": {}}


def _kernels():
    return DeviceKernels(torch.device("cuda:0"))


def _t(a):
    return torch.as_tensor(np.array(a)).cuda()                # a copy: the cached cases are read-only


def _layout(x, layout):
    """x on the device: dense, or a column slice of a wider matrix full of 1000s -- ld > D, neighbours must not leak in."""
    rows, D = x.shape
    if layout == "dense":
        return _t(x)
    off = 1 if layout == "slice_unaligned" else 4
    width = (off + D + 8) // 4 * 4 + (1 if layout == "slice_unaligned" else 0)
    big = torch.full((rows, width), 1000.0, device="cuda")
    big[:, off:off + D] = _t(x)
    t = big[:, off:off + D]
    assert t.stride(0) == width > D and (t.data_ptr() % 16 == 0) == (layout == "slice_aligned")
    return t


def _rel(dev, ref, scale):
    """max |dev - ref| / scale over the entries with a scale; where the scale is 0 the reference is an exact 0 and so must dev be."""
    dev, ref, scale = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (dev, ref, scale))
    dead = scale == 0
    assert not ref[dead].any() and not dev[dead].any(), "an exact zero of the reference is not zero on the device"
    return float(np.max(np.abs(dev - ref)[~dead] / scale[~dead])) if (~dead).any() else 0.0


# ---- 1. against double precision ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(rows, D, ties):
    x, c, s, w, time, event = cox_case(rows, D, ties)
    ref = cox_eval64(x, c, s, w, time, event)
    # what the scores' error may do to the residuals and the loss, relative to the gradient's and the loss's own scales
    smax = float(ref["score_scale"].max())
    live = ref["grad_scale"] > 0
    ec = (ref["e"] * ref["c"]) @ np.abs(ref["u"])
    kappa_g = float(np.max(2.0 * smax * ec[live] / ref["grad_scale"][live])) if live.any() else 0.0
    kappa_l = 2.0 * smax * float(event.sum()) / ref["loss_scale"] if ref["loss_scale"] > 0 else 0.0
    return ref, kappa_g, kappa_l


@functools.lru_cache(maxsize=None)
def _errors(rows, D, ties, layout):
    x, c, s, w, time, event = cox_case(rows, D, ties)
    ref, _, _ = _reference(rows, D, ties)
    k = _kernels()
    with k.cox_plan(time, event) as plan:
        loss, g, z = k.cox_eval(_layout(x, layout), c, s, w, plan, scores=True)
    z = z.cpu().numpy().astype(np.float64)
    assert g.dtype == np.float64 and g.shape == (D,) and z.shape == (rows,)
    assert np.isfinite(loss) and np.isfinite(g).all() and np.isfinite(z).all()
    return _rel(z, ref["scores"], ref["score_scale"]), _rel(g, ref["grad"], ref["grad_scale"]), _rel(loss, ref["loss"], ref["loss_scale"])


def _ceilings():
    refs = [_reference(rows, D, ties) for rows, D, ties in sorted({case[:3] for case in CASES})]
    kg, kl = max(r[1] for r in refs), max(r[2] for r in refs)
    return (GLM_RUN_ROWS + 9) * EPS + SCORE_CEILING * kg, 1e-13 + SCORE_CEILING * kl


def test_tolerances_are_inside_the_rounding_model():
    grad_ceiling, loss_ceiling = _ceilings()
    print(f"ceilings: scores {SCORE_CEILING:.3e}, gradient {grad_ceiling:.3e}, loss {loss_ceiling:.3e}")
    assert (SCORE_TOL, GRAD_TOL, LOSS_TOL) == (4 * SCORE_OBSERVED, 4 * GRAD_OBSERVED, 4 * LOSS_OBSERVED)
    assert SCORE_TOL <= SCORE_CEILING and GRAD_TOL <= grad_ceiling and LOSS_TOL <= loss_ceiling


@pytest.mark.parametrize("rows,D,ties,layout", CASES)
def test_cox_eval_vs_double(rows, D, ties, layout):
    es, eg, el = _errors(rows, D, ties, layout)
    print(f"cox_eval {rows}x{D} {ties} {layout}: scores {es:.3e}, gradient {eg:.3e}, loss {el:.3e}; "
          f"asserted {SCORE_TOL:.3e} / {GRAD_TOL:.3e} / {LOSS_TOL:.3e}")
    assert es <= SCORE_TOL and eg <= GRAD_TOL and el <= LOSS_TOL


def test_all_censored_and_a_single_event_row_are_exactly_zero():
    k = _kernels()
    x, c, s, w, time, event = cox_case(257, 130, "censored")
    with k.cox_plan(time, event) as plan:
        loss, g, _ = k.cox_eval(_t(x), c, s, w, plan)
    assert loss == 0.0 and not g.any()
    x, c, s, w, time, _ = cox_case(1, 5, "grid")
    with k.cox_plan(time, np.ones(1)) as plan:
        loss, g, _ = k.cox_eval(_t(x), c, s, w, plan)
    assert loss == 0.0 and not g.any()


@pytest.mark.parametrize("rows,D,ties", [(257, 130, "grid"), (100001, 8, "grid"), (100001, 8, "fifty")])
def test_loss_at_zero_weights_is_pure_scan_arithmetic(rows, D, ties):
    x, c, s, _, time, event = cox_case(rows, D, ties)
    ref = cox_eval64(x, c, s, np.zeros(D), time, event)
    k = _kernels()
    with k.cox_plan(time, event) as plan:
        loss, g, z = k.cox_eval(_t(x), c, s, np.zeros(D), plan, scores=True)
    rel = abs(loss - ref["loss"]) / ref["loss"]
    print(f"w = 0 at {rows}x{D} {ties}: loss {loss!r} against {ref['loss']!r}, relative error {rel:.3e}; gradient "
          f"{_rel(g, ref['grad'], ref['grad_scale']):.3e}")
    assert not z.any() and rel <= 1e-13
    assert _rel(g, ref["grad"], ref["grad_scale"]) <= (GLM_RUN_ROWS + 9) * EPS      # the scores are exact: the gradient's own roundings


# ---- 2. same bits, dropped columns, partial outputs, the plan -----------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [SHAPES[2], SHAPES[3], SHAPES[4]])
def test_same_bits_dropped_columns_and_partial_outputs(rows, D):
    x, c, s, w, time, event = cox_case(rows, D, "grid")
    s = s.copy()
    s[::3] = 0.0                                                  # every third column dropped
    t, k = _t(x), _kernels()
    with k.cox_plan(time, event) as plan:
        loss, g, z = k.cox_eval(t, c, s, w, plan, scores=True)
        loss2, g2, z2 = k.cox_eval(t, c, s, w, plan, scores=True)
        loss3, none, no_scores = k.cox_eval(t, c, s, w, plan, grad=False)
        loss4, g4, _ = k.cox_eval(t, c, s, w, plan)
    assert np.float64(loss).view(np.int64) == np.float64(loss2).view(np.int64) and np.array_equal(g.view(np.int64), g2.view(np.int64))
    assert torch.equal(z.view(torch.int32), z2.view(torch.int32))
    assert none is None and no_scores is None and loss3 == loss and loss4 == loss and np.array_equal(g.view(np.int64), g4.view(np.int64))
    assert not g[::3].any() and g[1::3].all()
    ref = cox_eval64(x, c, s, w, time, event)
    live = ref["grad_scale"] > 0
    assert _rel(g[live], ref["grad"][live], ref["grad_scale"][live]) <= GRAD_TOL
    # the scores are what the GLM predictor gives for the same weights and a zero bias
    W = np.concatenate([w, [0.0]])[None, :].astype(np.float32)
    _, _, zg = k.glm_eval(t, c, s, None, W, [SQUARED], grad=False, scores=True)
    assert torch.equal(z, zg[:, 0])


def test_plan_lifetime_and_argument_errors():
    k = _kernels()
    x, c, s, w, time, event = cox_case(33, 6, "grid")
    plan = k.cox_plan(time, event)
    assert plan.rows == 33 and not plan.closed
    with pytest.raises(ValueError, match="33 rows"):
        k.cox_eval(_t(x[:20]), c, s, w, plan)                     # another row count than the plan's
    with pytest.raises(ValueError):
        k.cox_eval(torch.zeros((33, 8193), device="cuda"), np.zeros(8193), np.ones(8193), np.zeros(8193), plan)
    plan.close()
    plan.close()
    assert plan.closed
    with pytest.raises(ValueError, match="closed"):
        k.cox_eval(_t(x), c, s, w, plan)
    for bad_time, bad_event in ((np.where(np.arange(33) == 5, np.nan, time), event), (time, np.where(np.arange(33) == 5, 2.0, event))):
        with pytest.raises(ValueError):
            k.cox_plan(bad_time, bad_event)
    del plan
    k.cox_plan(time, event)                                       # never closed: the finalizer destroys it


def test_a_plan_serves_a_call_under_another_stream():
    """The plan's calls run on the stream it was made on; inputs uploaded under another current stream are waited for."""
    k = _kernels()
    x, c, s, w, time, event = cox_case(515, 5142, "grid")
    t = _t(x)
    with k.cox_plan(time, event) as plan:
        loss, g, z = k.cox_eval(t, c, s, w, plan, scores=True)
        with torch.cuda.stream(torch.cuda.Stream()):
            loss2, g2, z2 = k.cox_eval(t, c, s, w, plan, scores=True)
            z2 = z2.cpu()
    assert loss2 == loss and np.array_equal(g.view(np.int64), g2.view(np.int64)) and torch.equal(z.cpu(), z2)


# ---- 3. concordance -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conc_case(n):
    rs = np.random.default_rng(977 * n + 1)
    time = (30.0 * rs.integers(1, max(2, min(n // 3, 400)) + 1, n)).astype(np.float32)      # ties in time ...
    risk = (rs.integers(-40, 41, n) / 8.0).astype(np.float32)                               # ... and in risk
    event = (rs.random(n) < 0.6).astype(np.float32)
    return time, event, risk, SV.concordance_counts(time, event, risk)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, CONC_I_TILE + 1, CONC_J_CHUNK + 1, 20001])
def test_concordance_counts_equal_the_hosts(n):
    time, event, risk, want = _conc_case(n)
    got = _kernels().concordance(time, event, risk)
    print(f"concordance n = {n}: {got}")
    assert got == want and got[0] == got[1] + got[2] + got[3]
    if n >= 63:
        assert min(want) > 0                                      # every count is exercised
    assert _kernels().concordance(_t(time), _t(event), _t(risk)) == want      # device tensors are taken as they are


def test_concordance_all_censored_is_all_zeros():
    time, _, risk, _ = _conc_case(CONC_J_CHUNK + 1)
    assert _kernels().concordance(time, np.zeros_like(time), risk) == (0, 0, 0, 0)


# ---- 4. the fit -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_fit():
    x, c, s, _, time, event = cox_case(257, 130, "grid")
    k, t = _kernels(), _t(x)
    n, l2 = 257.0, 1e-2
    with k.cox_plan(time, event) as plan:
        fit = SV.fit_cox(lambda w: k.cox_eval(t, c, s, w, plan)[:2], 130, n, l2)
    g = penalised_cox_gradient64(x, c, s, fit["w"], time, event, n, l2)
    return fit, float(np.abs(g).max())


def test_device_fit_reaches_the_optimum():
    fit, gnorm = _device_fit()
    print(f"device Cox fit: {fit['iterations']} iterations, converged {fit['converged']}, device |g|_inf {fit['grad_inf_norm']:.3e}, "
          f"float64 |g|_inf at its w {gnorm:.3e}; asserted {4 * FIT_OBSERVED:.3e}")
    assert np.isfinite(fit["w"]).all() and fit["iterations"] >= 5
    assert gnorm <= 4 * FIT_OBSERVED                              # |w - w*| <= gnorm / l2: strongly convex


# ---- 5. end to end on planted cohorts ------------------------------------------------------------------------------------------------
def _cohorts():
    return planted_survival(600, 130, 3), planted_survival(600, 130, 7), planted_survival(300, 130, 11)


@functools.lru_cache(maxsize=None)
def _both(permuted):
    (train, train_s), (synth, synth_s), (test, test_s) = _cohorts()
    if permuted:
        synth_s = synth_s[np.random.default_rng(0).permutation(len(synth_s))]
    dev = BiologicalValidator(CONF).survival_utility(train, train_s, synth, synth_s, test, test_s)
    t = lambda a: torch.from_numpy(np.array(a))
    return dev, survival_metrics(SurvivalNumpyKernels(), t(train), train_s, t(synth), synth_s, t(test), test_s)


@pytest.mark.parametrize("permuted", [False, True])
def test_survival_utility_vs_float64_pipeline(permuted):
    dev, ref = _both(permuted)
    assert set(dev) == set(ref) == {"survival_tstr_cindex", "survival_trtr_cindex", "survival_cindex_gap", "survival_coef_cosine",
                                    "survival_comparable_pairs", "survival_event_share_real_train", "survival_event_share_synthetic",
                                    "survival_event_share_real_test"}
    worst = max(abs(dev[key] - ref[key]) for key in ("survival_tstr_cindex", "survival_trtr_cindex", "survival_cindex_gap"))
    print(f"survival_utility permuted={permuted}: max |d C-index| = {worst:.3e}, |d cosine| = "
          f"{abs(dev['survival_coef_cosine'] - ref['survival_coef_cosine']):.3e}; asserted {4 * E2E_OBSERVED:.3e}", dev)
    assert worst <= 4 * E2E_OBSERVED
    assert all(dev[key] == ref[key] for key in ref if key.startswith("survival_event_share_") or key == "survival_comparable_pairs")
    assert abs(dev["survival_coef_cosine"] - ref["survival_coef_cosine"]) <= 1e-3


def test_permuted_survival_loses_the_concordance_and_nothing_else():
    good, bad = _both(False)[0], _both(True)[0]
    assert good["survival_trtr_cindex"] >= 0.70 and good["survival_tstr_cindex"] >= 0.70 and abs(good["survival_cindex_gap"]) <= 0.05
    assert 0.40 <= bad["survival_tstr_cindex"] <= 0.60
    assert good["survival_trtr_cindex"] == bad["survival_trtr_cindex"]      # trained on the same real rows: the same bits


def test_validate_all_adds_the_keys_only_when_asked():
    import pandas as pd
    def frames(n, seed):
        x, surv = planted_survival(n, 52, seed)
        m = pd.DataFrame((x[:, :20] > 0).astype(np.float32), columns=[f"M{i}" for i in range(20)])
        e = pd.DataFrame(x[:, 20:50], columns=[f"G{i}" for i in range(30)])
        p = pd.DataFrame(x[:, 50:52], columns=["PW0", "PW1"])
        return m, e, p, surv
    rm, re_, rp, rs = frames(200, 3)
    sm, se, sp, ss = frames(240, 4)
    tm, te, tp, ts = frames(150, 5)
    val = BiologicalValidator(CONF)
    np.random.seed(0)
    plain = val.validate_all(rm, re_, rp, sm, se, sp)
    np.random.seed(0)
    full = val.validate_all(rm, re_, rp, sm, se, sp, survival=(rs, ss, (tm, te, tp), ts))
    extra = set(full) - set(plain)
    assert extra == {"survival_tstr_cindex", "survival_trtr_cindex", "survival_cindex_gap", "survival_coef_cosine",
                     "survival_comparable_pairs", "survival_event_share_real_train", "survival_event_share_synthetic",
                     "survival_event_share_real_test"}
    assert all(abs(full[key] - plain[key]) <= 1e-9 * max(1.0, abs(plain[key])) for key in plain)      # (the MMD's double atomics: last bits)
    assert all(np.isfinite(full[key]) for key in extra)
    with pytest.raises(ValueError, match="survival="):
        val.validate_all(rm, re_, rp, sm, se, sp, survival=(rs, ss))


def test_sharded_validator_raises():
    x, s = planted_survival(60, 8, 3)
    sharded = BiologicalValidator(CONF, sharded=True)
    with pytest.raises(NotImplementedError, match="sharded.*risk set"):
        sharded.survival_utility(x, s, x, s, x, s)
