"""GPU: the univariate Cox screen kernel (osd_val_cox_score: coxs_pass, coxs_scan, coxs_reduce, csrc/cox_score.hip), the driver and
screen of survival.py over it and ``BiologicalValidator.prognostic_fidelity`` above them, against the float64 restatement of
tests/prognostic_helpers.py evaluated on the same fp32 inputs.

Shapes (rows, D), R = OSD_COXS_ROWS = 128: (1, 5), (33, 6), (257, 130), (R - 1, 3), (R, 3), (2 R + 1, 62), (515, 5142) -- one row; one
ragged block; three blocks with a one-row tail and a ragged slab; a block one short of full, exactly full, two blocks and a row; five
blocks by 21 slabs, the last slab 22 columns wide, D % 4 == 2.  Every shape in the three layouts of test_gpu_survival.py (dense,
aligned slice, unaligned slice) on a 30-day grid of times.  No D here is a multiple of 4, so only the aligned slice (ld % 4 == 0)
takes the 16-byte load path; the dense matrix and the unaligned slice take the dword path.  (257, 130) also with distinct times,
all times equal, all censored (exact zeros) and all events; (2 R + 1, 62) also with only 50 distinct times, so that both block
boundaries fall inside tie groups.  Every case at beta = 0 (a NULL beta: the path without exp) and at beta uniform in [-1, 1] with the
bound the beta = 0 call's own absmax gave.

  * loglik, score and info against float64, each error normalised by the sum of the absolute values of the terms the sum adds and
    subtracts (per event |beta u - k| + |log A0|; |u| + |A1 / A0|; A2 / A0 + (A1 / A0)^2); where that is 0 (all censored, a dropped
    column) the device must give the reference's exact 0.  absmax must be EQUAL: a maximum of the same doubles.

    Measured, the largest over the cases, at beta = 0: loglik 1.928e-15 (257 x 130, all events), score 6.314e-16 (257 x 130, one
    time), info 6.754e-15 (515 x 5142); at beta != 0: loglik 1.764e-15, score 3.101e-15, info 5.729e-15 (all at 515 x 5142).  The
    three layouts of a shape give the same figures, and test_the_three_layouts_give_the_same_bits asserts that their outputs are
    the same bits.  Asserted: 4 x the measured figures (TOL is OBSERVED times 4 by construction; what the rounding-model test checks
    is that TOL stays under the ceilings below, which are about 15 x TOL: the model bounds the worst case, so it constrains little).
    It may not exceed what the rounding model allows.  With eps = 2^-53 and n the rows, a column's running sums A0, A1, A2 are chains of
    at most n additions of terms with at most 6 roundings of their own, and e = exp(beta u - k) adds the exponent's error
    (6 max |beta| R eps: u has two roundings, the product, the shift and the difference one each) and exp's documented 1 ulp (the
    HIP math API's accuracy table: double exp and log, 1 ulp each): rs = (n + 8) eps + [2^-52 + 6 max |beta| R eps], the bracket
    only at beta != 0.  That error is relative to the sums of ABSOLUTE terms, B1 = sum e |u| for A1.  An output is a chain of at
    most 3 n + 64 additions (two per position, the block partials, the runs), so relative to its scale:
      loglik  (3 n + 64) eps + 2^-52 [log] + (rs + 6 max |beta| R eps) events / scale
      score   (3 n + 67) eps + rs (1 + sum_p delta_p (B1 / A0) / scale)
      info    (3 n + 68) eps + 2 rs (1 + sum_p delta_p |A1 / A0| (B1 / A0) / scale)
    with the condition factors (events / scale and the two spreads) taken from the float64 reference of the tested data, and the whole
    doubled, because the float64 reference is itself a chain of the same length with the same 1-ulp exp and log.  Over the cases
    the ceilings come to 3.8e-13 / 6.0e-13 / 6.2e-13 at beta = 0 and 3.8e-13 / 6.2e-13 / 7.4e-13 at beta != 0; every case is also held
    to its own ceiling (1.5e-14 for the single row).
  * censored cohorts and a single event row at beta = 0: exact zeros.  A column with scale 0: exact zeros, and every other column keeps
    its bits.
  * at beta = 0 the score is minus the gradient of osd_val_cox_eval at w = 0 within that kernel's asserted gradient tolerance
    (test_gpu_survival.py: 4 x 1.347e-7 of grad_scale).  Measured: 2.8e-8, 2.4e-8 and 2.2e-8 -- the fp32 gradient's own rounding.
  * the same bits on a second call, and per column between a call on a whole matrix that takes the 16-byte path (an aligned slice of
    a wider one; at (257, 132) the dense matrix too), one on a column slice of it (another base, ld > D, dword loads) and one on the
    dense matrix; and between the three layouts of every shape.
  * the screen on the planted cohort (600 x 130): the device's hits are the float64 screen's, and its effects differ by at most 1.443e-15
    (measured with the one-step estimate; 4.4e-16 with the Newton iterations; z by 2.0e-14; asserted 4 x that).
  * ``prognostic_fidelity`` reproduces the set equalities of test_prognostic_cpu.py; ``validate_all`` gains the ``prog_`` keys only
    when asked; a sharded validator raises."""
import functools

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import survival as SV
from osteosarcoma_diffusionmodel_amd.validation import COXS_ROWS, BiologicalValidator, DeviceKernels, prognostic_metrics
from prognostic_helpers import PrognosticNumpyKernels, cox_score64
from survival_helpers import cox_case, cox_eval64, planted_survival

pytestmark = pytest.mark.gpu

R = COXS_ROWS
SHAPES = [(1, 5), (33, 6), (257, 130), (R - 1, 3), (R, 3), (2 * R + 1, 62), (515, 5142)]
LAYOUTS = ["dense", "slice_aligned", "slice_unaligned"]
CASES = ([(rows, D, "grid", layout) for rows, D in SHAPES for layout in LAYOUTS] +
         [(257, 130, ties, "dense") for ties in ("distinct", "equal", "censored", "events")] + [(2 * R + 1, 62, "fifty", "dense")])
MODES = ["zero", "beta"]
FIELDS = ("loglik", "score", "info")
EPS = 2.0 ** -53
ULP = 2.0 ** -52                  # the documented bound of the device's double exp and log: 1 ulp
OBSERVED = {"zero": (1.928e-15, 6.314e-16, 6.754e-15), "beta": (1.764e-15, 3.101e-15, 5.729e-15)}      # measured maxima over CASES: loglik, score, info
TOL = {mode: tuple(4 * v for v in vals) for mode, vals in OBSERVED.items()}
GRAD_TOL = 4 * 1.347e-7           # test_gpu_survival.py: osd_val_cox_eval's gradient against float64, of grad_scale
EFFECT_OBSERVED = 1.443e-15        # measured max |device effect - float64 effect| on the planted cohort
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


def _beta(D):
    return np.random.default_rng(7919 * D + 1).uniform(-1.0, 1.0, D)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. against double precision ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(rows, D, ties, mode):
    x, c, s, _, time, event = cox_case(rows, D, ties)
    zero = cox_score64(x, c, s, time, event)
    if mode == "zero":
        return zero, None, None
    # the bound is the device's own absmax of the beta = 0 call: test_cox_score_vs_double holds it EQUAL to the reference's, bit for bit
    beta, bound = _beta(D), zero["absmax"]
    return cox_score64(x, c, s, time, event, beta, bound), beta, bound


@functools.lru_cache(maxsize=None)
def _device(rows, D, ties, layout, mode):
    x, c, s, _, time, event = cox_case(rows, D, ties)
    _, beta, bound = _reference(rows, D, ties, mode)
    k, t = _kernels(), _layout(x, layout)
    with k.cox_plan(time, event) as plan:
        out = k.cox_score(t, c, s, plan, beta=beta, bound=bound, absmax=True)
    assert all(v.dtype == np.float64 and v.shape == (D,) and np.isfinite(v).all() for v in out)
    return out


def _ceilings(rows, D, ties, mode):
    ref, beta, bound = _reference(rows, D, ties, mode)
    shift = float(np.abs(beta * bound).max()) if mode == "beta" else 0.0
    rs = (rows + 8) * EPS + ((ULP + 6 * shift * EPS) if mode == "beta" else 0.0)
    worst = lambda num, den: float(np.max(num[den > 0] / den[den > 0])) if (den > 0).any() else 0.0
    kl = worst(np.full(D, ref["events"]), ref["loglik_scale"])
    ks, ki = worst(ref["spread1"], ref["score_scale"]), worst(ref["spread2"], ref["info_scale"])
    return (2 * ((3 * rows + 64) * EPS + ULP + (rs + 6 * shift * EPS) * kl), 2 * ((3 * rows + 67) * EPS + rs * (1 + ks)),
            2 * ((3 * rows + 68) * EPS + 2 * rs * (1 + ki)))


@pytest.mark.parametrize("mode", MODES)
def test_tolerances_are_inside_the_rounding_model(mode):
    per_case = [_ceilings(rows, D, ties, mode) for rows, D, ties in sorted({case[:3] for case in CASES})]
    ceilings = tuple(max(c[i] for c in per_case) for i in range(3))      # (every case is also held to its OWN ceiling, below)
    print(f"{mode}: ceilings loglik {ceilings[0]:.3e}, score {ceilings[1]:.3e}, info {ceilings[2]:.3e}; asserted {TOL[mode]}")
    assert all(t <= c for t, c in zip(TOL[mode], ceilings))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D,ties,layout", CASES)
def test_cox_score_vs_double(rows, D, ties, layout, mode):
    ref, _, _ = _reference(rows, D, ties, mode)
    ll, sc, info, absmax = _device(rows, D, ties, layout, mode)
    errs = tuple(_rel(dev, ref[name], ref[name + "_scale"]) for name, dev in zip(FIELDS, (ll, sc, info)))
    print(f"cox_score {rows}x{D} {ties} {layout} {mode}: loglik {errs[0]:.3e}, score {errs[1]:.3e}, info {errs[2]:.3e}; "
          f"asserted {TOL[mode][0]:.3e} / {TOL[mode][1]:.3e} / {TOL[mode][2]:.3e}")
    assert np.array_equal(_bits(absmax), _bits(ref["absmax"]))
    assert all(e <= t for e, t in zip(errs, TOL[mode]))
    assert all(e <= c for e, c in zip(errs, _ceilings(rows, D, ties, mode)))      # and inside this case's own rounding model


@pytest.mark.parametrize("mode", MODES)
def test_censored_cohorts_and_a_single_event_row_are_exactly_zero(mode):
    ll, sc, info, absmax = _device(257, 130, "censored", "dense", mode)
    assert not ll.any() and not sc.any() and not info.any() and absmax.all()
    if mode == "zero":
        k = _kernels()
        x, c, s, _, time, _ = cox_case(1, 5, "grid")
        with k.cox_plan(time, np.ones(1)) as plan:
            ll, sc, info, _ = k.cox_score(_t(x), c, s, plan)
        assert not ll.any() and not sc.any() and not info.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D", [(257, 130), (2 * R + 1, 62)])
def test_a_dropped_column_is_exactly_zero_and_moves_no_other_bit(rows, D, mode):
    x, c, s, _, time, event = cox_case(rows, D, "grid")
    _, beta, bound = _reference(rows, D, "grid", mode)
    full = _device(rows, D, "grid", "dense", mode)
    s2 = s.copy()
    s2[::3] = 0.0                                                 # every third column dropped
    k = _kernels()
    with k.cox_plan(time, event) as plan:
        got = k.cox_score(_t(x), c, s2, plan, beta=beta, bound=bound, absmax=True)
    keep = np.arange(D) % 3 != 0
    for a, b in zip(got, full):
        assert not a[~keep].any() and np.array_equal(_bits(a[keep]), _bits(b[keep]))
    assert all(full[i][~keep].any() for i in range(3))


# ---- 2. the score at 0 and osd_val_cox_eval's gradient at w = 0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,ties", [(257, 130, "grid"), (2 * R + 1, 62, "fifty"), (515, 5142, "grid")])
def test_score_at_zero_is_minus_the_cox_eval_gradient(rows, D, ties):
    x, c, s, _, time, event = cox_case(rows, D, ties)
    ref = cox_eval64(x, c, s, np.zeros(D), time, event)
    k, t = _kernels(), _t(x)
    with k.cox_plan(time, event) as plan:
        _, g, _ = k.cox_eval(t, c, s, np.zeros(D), plan)
        _, sc, _, _ = k.cox_score(t, c, s, plan)
    err = _rel(sc, -g, ref["grad_scale"])
    print(f"score + grad at {rows}x{D} {ties}: {err:.3e} of grad_scale; asserted {GRAD_TOL:.3e}")
    assert err <= GRAD_TOL


# ---- 3. same bits -------------------------------------------------------------------------------------------------------------------
def _quad_path(t):
    """osd_val_cox_score's host rule: the 16-byte load path where the base is 16-byte aligned, ld % 4 == 0 and ld holds the last quad."""
    ld, D = t.stride(0), t.shape[1]
    return t.data_ptr() % 16 == 0 and ld % 4 == 0 and ld >= (D + 3) // 4 * 4


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D", SHAPES)
def test_the_three_layouts_give_the_same_bits(rows, D, mode):
    """The aligned slice takes the 16-byte path, the unaligned slice the dword path, and so does the dense matrix at these D (none is a
    multiple of 4): a column's bits may not depend on the path, the base or ld."""
    x = cox_case(rows, D, "grid")[0]
    assert D % 4 and [_quad_path(_layout(x, layout)) for layout in LAYOUTS] == [False, True, False]
    dense, quad, dword = (_device(rows, D, "grid", layout, mode) for layout in LAYOUTS)
    for a, b, c in zip(dense, quad, dword):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,D", [(257, 130), (257, 132), (515, 5142)])
def test_same_bits_on_a_second_call_and_on_a_column_slice(rows, D, mode):
    """A whole-matrix call on the 16-byte path, twice, against a call on a column slice of the SAME matrix on the dword path (another
    base, ld > D), which moves every column to another lane -- and against the dense matrix, which takes the 16-byte path only at
    D = 132 (at D % 4 == 2 its ld is no multiple of 4)."""
    x, c, s, _, time, event = cox_case(rows, D, "grid")
    _, beta, bound = _reference(rows, D, "grid", mode)
    k, dense, whole = _kernels(), _t(x), _layout(x, "slice_aligned")
    lo, hi = 1, D - 2
    part = whole[:, lo:hi]
    assert _quad_path(whole) and not _quad_path(part) and part.data_ptr() % 16 != 0 and part.stride(0) == whole.stride(0) > D
    assert _quad_path(dense) == (D % 4 == 0)
    cut = lambda v: None if v is None else v[lo:hi]
    with k.cox_plan(time, event) as plan:
        a = k.cox_score(whole, c, s, plan, beta=beta, bound=bound, absmax=True)
        b = k.cox_score(whole, c, s, plan, beta=beta, bound=bound, absmax=True)
        d = k.cox_score(dense, c, s, plan, beta=beta, bound=bound, absmax=True)
        p = k.cox_score(part, c[lo:hi], s[lo:hi], plan, beta=cut(beta), bound=cut(bound), absmax=True)
    for u, v, w, q in zip(a, b, d, p):
        assert np.array_equal(_bits(u), _bits(v)) and np.array_equal(_bits(u), _bits(w)) and np.array_equal(_bits(u[lo:hi]), _bits(q))


# ---- 4. arguments ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_refused():
    k = _kernels()
    x, c, s, _, time, event = cox_case(33, 6, "grid")
    t = _t(x)
    cd, sd = _t(c), _t(s)
    o = torch.zeros((3, 8200), dtype=torch.float64, device="cuda")
    p = L.ptr
    with k.cox_plan(time, event) as plan:
        call = lambda rows, ld, D, outs: L.lib().osd_val_cox_score(plan.handle, p(t), rows, ld, D, p(cd), p(sd), None, None, *outs, None)
        good = [p(o[0]), p(o[1]), p(o[2])]
        assert call(33, 6, 6, good) == L.OSD_OK
        assert call(20, 6, 6, good) == L.OSD_EINVAL and b"33 rows" in L.lib().osd_last_error()
        assert call(33, 6, 0, good) == L.OSD_EINVAL and call(33, 8193, 8193, good) == L.OSD_EINVAL and call(33, 5, 6, good) == L.OSD_EINVAL
        for hole in range(3):
            outs = list(good)
            outs[hole] = None
            assert call(33, 6, 6, outs) == L.OSD_EINVAL
        with pytest.raises(ValueError, match="33 rows"):
            k.cox_score(_t(x[:20]), c, s, plan)
        with pytest.raises(ValueError, match="beta"):
            k.cox_score(t, c, s, plan, beta=np.zeros(5))
    with pytest.raises(ValueError, match="closed"):
        k.cox_score(t, c, s, plan)


# ---- 5. the screen, the validator ----------------------------------------------------------------------------------------------------
def _hits(scr, alpha=0.05):
    return set(np.nonzero(scr["q"] < alpha)[0].tolist())


@functools.lru_cache(maxsize=None)
def _screens(mle):
    x, surv = planted_survival(600, 130, 3)
    center = x.astype(np.float64).mean(0).astype(np.float32)
    scale = (1.0 / x.astype(np.float64).std(0, ddof=1)).astype(np.float32)
    k, kn = _kernels(), PrognosticNumpyKernels()
    with k.cox_plan(surv[:, 0], surv[:, 1]) as plan:
        dev = SV.cox_screen(k, _t(x), plan, center, scale, mle=mle)
    with kn.cox_plan(surv[:, 0], surv[:, 1]) as plan:
        ref = SV.cox_screen(kn, torch.from_numpy(np.array(x)), plan, center, scale, mle=mle)
    return dev, ref


@pytest.mark.parametrize("mle", [True, False])
def test_device_screen_vs_float64_screen(mle):
    dev, ref = _screens(mle)
    gap = float(np.abs(dev["effect"] - ref["effect"]).max())
    print(f"screen mle={mle}: max |d effect| = {gap:.3e}, max |d z| = {np.abs(dev['z_score'] - ref['z_score']).max():.3e}; "
          f"asserted {4 * EFFECT_OBSERVED:.3e}")
    assert _hits(dev) == _hits(ref) == {0, 1, 2, 3}
    assert gap <= 4 * EFFECT_OBSERVED
    assert np.array_equal(dev["converged"], ref["converged"]) and dev["converged"].all()
    assert np.array_equal(dev["absmax"], ref["absmax"])


@functools.lru_cache(maxsize=None)
def _fidelity(permuted):
    (real, real_s), (synth, synth_s) = planted_survival(600, 130, 3), planted_survival(600, 130, 7)
    if permuted:
        synth_s = synth_s[np.random.default_rng(0).permutation(len(synth_s))]
    dev = BiologicalValidator(CONF).prognostic_fidelity(real, real_s, synth, synth_s, return_rows=True)
    t = lambda a: torch.from_numpy(np.array(a))
    return dev, prognostic_metrics(PrognosticNumpyKernels(), t(real), real_s, t(synth), synth_s)


def test_prognostic_fidelity_on_planted_cohorts():
    (out, rows), (ref, _) = _fidelity(False)
    (bad, bad_rows), _ = _fidelity(True)
    print(out, bad)
    assert set(out) == set(ref)
    assert _hits(rows["real"]) == {0, 1, 2, 3} and _hits(rows["synthetic"]) == {0, 1, 2, 3}
    assert np.abs(rows["real"]["effect"][:4] - np.array([0.58, -0.64, 0.30, -0.30])).max() <= 0.01
    assert out["prog_precision"] == 1.0 and out["prog_recall"] == 1.0 and out["prog_real_hits"] == 4 and out["prog_synth_hits"] == 4
    assert _hits(bad_rows["synthetic"]) == set() and bad["prog_recall"] == 0.0 and abs(bad["prog_effect_slope"]) < 0.05
    for key in ("prog_features", "prog_constant_features", "prog_not_converged_real", "prog_not_converged_synth", "prog_events_real",
                "prog_events_synth", "prog_real_hits", "prog_synth_hits", "prog_max_gap_feature"):
        assert out[key] == ref[key]
    assert abs(out["prog_effect_slope"] - ref["prog_effect_slope"]) <= 1e-6 and abs(out["prog_max_abs_z_real"] - ref["prog_max_abs_z_real"]) <= 1e-6


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
    val = BiologicalValidator(CONF)
    np.random.seed(0)
    plain = val.validate_all(rm, re_, rp, sm, se, sp)
    np.random.seed(0)
    full = val.validate_all(rm, re_, rp, sm, se, sp, prognostic=(rs, ss))
    extra = set(full) - set(plain)
    assert extra and all(key.startswith("prog_") for key in extra)
    assert {"prog_effect_slope", "prog_recall", "prog_features", "prog_events_synth", "prog_effect_pearson_mutations",
            "prog_effect_pearson_expression", "prog_effect_pearson_pathways"} <= extra
    assert full["prog_features"] == 52 and full["prog_events_real"] == int(rs[:, 1].sum())
    assert all(abs(full[key] - plain[key]) <= 1e-9 * max(1.0, abs(plain[key])) for key in plain)      # (the MMD's double atomics: last bits)
    with pytest.raises(ValueError, match="prognostic="):
        val.validate_all(rm, re_, rp, sm, se, sp, prognostic=(rs,))


def test_sharded_validator_and_censored_cohorts_raise():
    x, s = planted_survival(60, 8, 3)
    with pytest.raises(ValueError, match="sharded.*risk set"):
        BiologicalValidator(CONF, sharded=True).prognostic_fidelity(x, s, x, s)
    censored = s.copy()
    censored[:, 1] = 0.0
    with pytest.raises(ValueError, match="synthetic cohort has no event"):
        BiologicalValidator(CONF).prognostic_fidelity(x, s, x, censored)
