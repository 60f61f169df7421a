"""GPU: the regularised-linear-model kernel (osd_val_glm_eval: glm_kernel + glm_reduce, csrc/glm.hip), the column moments beside it, and
``BiologicalValidator.downstream_utility`` / ``discriminator_test`` above them, against the float64 restatement of
tests/utility_helpers.py evaluated on the same fp32 inputs.

Shapes (rows, D, K): (1, 5, 1), (33, 6, 1), (257, 130, 3), (1000, 258, 4), (515, 5142, 3), (100001, 8, 2) -- one row; row tails; D below
one 16-byte vector per lane; D % 4 == 2 (130, 258, 5142); the reference's width (three column quads per lane, seven waves); every K.
A call's rows are cut into at most 768 contiguous work items of at least 16 rows, so the first five shapes have one fp32 run per item;
(100001, 8, 2) is the shape whose items have MORE THAN ONE RUN AND A RAGGED LAST ONE: 758 items of 132 rows = a run of
OSD_GLM_RUN_ROWS = 128 rows folded into the item's double sums, then one of 4, and a last item of 77 rows.  Dense, its eight columns take
the 16-byte path; the dense layouts of the other shapes (ld % 4 != 0) and every unaligned slice take the dword path, and the aligned
slices of D % 4 == 2 read a last vector that straddles D.

  * integers (squared heads, integer X, centres, W, y and row weights, scale 1): every product and run sum is an integer below 2^24,
    so 2 x loss and the gradient must EQUAL the int64 result -- a dropped, doubled or unmasked row or column is a wrong integer;
  * real-valued data, logistic and squared heads mixed: loss, gradient and scores against float64, each error normalised by its
    natural scale (sum |a l|; sum |a f u| per column; sum |w u| + |bias| per score).

    Measured, the largest over the shapes and layouts: scores 2.117e-7 (100001 x 8, whose two small weights per head cancel),
    gradient 7.225e-8 and loss 3.991e-8 (both at 1 x 5); at 515 x 5142 1.3e-8, 3.8e-8 and 2.2e-8; the extreme-logit case below, held
    to the same tolerances: 1.4e-7, 1.0e-7 and 8e-10.  Asserted: 4 x that -- other seeds, and the freedom of the summation order inside a run.  It may not exceed what
    the rounding model allows: one rounding per centred value, per product (w x scale, then w' x d) and per accumulate -- at most 16
    terms in a lane, 6 butterfly steps, 8 waves and the bias: SCORE_CEILING = 34 x 2^-24; for a gradient entry one rounding per
    centred value, three for the residual a (sigma(z) - y), four ulp for exp, log1p and the division, one per product and per
    accumulate within a run, double above: (OSD_GLM_RUN_ROWS + 9) x 2^-24, plus what the score's error does to the residual,
    |d f| <= a |d z|: SCORE_CEILING x kappa with kappa = sum a S |u| / sum |a f u| (S the score's own scale), taken from the float64
    reference of the tested data; the loss the same way with |d l| <= |f| |d z|.
  * fits: the float64 gradient of the penalised objective at the W the device fit returns.  Measured at 257 x 130, K = 3, l2 = 1e-2:
    |g|_inf = 7.647e-5 after 137 iterations (the device's own gradient says 7.645e-5) -- the fit ends at the noise floor of an
    objective whose row terms are fp32, above the default tol of 1e-5, and reports converged=False.  Asserted: 4 x that.  The
    objective is strongly convex, so |W - W*| <= that / l2 whatever path the optimiser took.
  * end to end: |d AUC| and |d R^2| between the validator and the float64 pipeline (same driver, float64 kernels).  Measured: 1.7e-8
    (faithful cohort), 6.675e-6 (permuted conditions, a fit of noise), 2.4e-9 (classifier two-sample test), 1.1e-8 (two row shards
    against one process).  Asserted: 4 x the largest."""
import ctypes as C_
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import utility as U
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import (GLM_RUN_ROWS, BiologicalValidator, DeviceKernels, c2st_metrics, glm_sums,
                                                        utility_metrics)
from utility_helpers import (C2ST_SEEDS, LOGISTIC, SQUARED, NumpyKernels, glm_case, glm_eval64, penalised_gradient64, planted)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 1), (33, 6, 1), (257, 130, 3), (1000, 258, 4), (515, 5142, 3), (100001, 8, 2)]
LAYOUTS = ["dense", "slice_aligned", "slice_unaligned"]
EPS = 2.0 ** -24
SCORE_OBSERVED, GRAD_OBSERVED, LOSS_OBSERVED = 2.117e-7, 7.225e-8, 3.991e-8      # measured maxima over SHAPES x LAYOUTS
SCORE_TOL, GRAD_TOL, LOSS_TOL = 4 * SCORE_OBSERVED, 4 * GRAD_OBSERVED, 4 * LOSS_OBSERVED
SCORE_CEILING = 34 * EPS
FIT_OBSERVED = 7.647e-5           # measured |float64 penalised gradient|_inf at the device fit's W
E2E_OBSERVED = 6.675e-6           # measured max |d AUC|, |d R^2| of the validator against the float64 pipeline
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


# ---- 1. integers: exact ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_case(rows, D, K):
    rs = np.random.default_rng(131 * rows + 7 * D + K)
    x = rs.integers(0, 5, (rows, D))
    c = np.where(np.arange(D) % 3 == 1, 2, 0)
    W = rs.integers(-2, 3, (K, D + 1)) * (rs.random((K, D + 1)) < min(1.0, 24.0 / D))      # about 24 non-zero weights per head
    y = rs.integers(-3, 4, (rows, K))
    a = rs.integers(0, 4, rows)                                                            # weight 0 included
    d = x - c
    z = d @ W[:, :D].T + W[:, D]
    f = (z - y) * a[:, None]
    grad = f.T @ np.concatenate([d, np.ones((rows, 1), dtype=np.int64)], axis=1)
    loss2 = (a[:, None] * (z - y) ** 2).sum(0)
    # every fp32 intermediate is an integer below 2^24: partial dots, residuals, row losses and any run of up to GLM_RUN_ROWS terms
    assert (np.abs(d) @ np.abs(W[:, :D]).T + np.abs(W[:, D])).max() < 2 ** 24
    assert np.abs(a[:, None] * (z - y) ** 2).max() < 2 ** 24
    assert GLM_RUN_ROWS * np.abs(f).max() * np.abs(d).max() < 2 ** 24
    return x.astype(np.float32), c.astype(np.float32), W.astype(np.float32), y.astype(np.float32), a.astype(np.float32), z, grad, loss2


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,D,K", SHAPES)
def test_exact_on_integers(rows, D, K, layout):
    x, c, W, y, a, z, grad, loss2 = _int_case(rows, D, K)
    loss, g, s = _kernels().glm_eval(_layout(x, layout), c, np.ones(D, dtype=np.float32), y, W, [SQUARED] * K, row_weight=a, scores=True)
    assert g.dtype == np.float64 and g.shape == (K, D + 1) and s.dtype == torch.float32 and tuple(s.shape) == (rows, K)
    assert np.array_equal(s.cpu().numpy().astype(np.int64), z) and np.array_equal(s.cpu().numpy(), z.astype(np.float32))
    assert np.array_equal(g, grad.astype(np.float64)), f"{int((g != grad).sum())} of {g.size} gradient entries differ"
    assert np.array_equal(2.0 * loss, loss2.astype(np.float64))


# ---- 2. against double precision ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(rows, D, K):
    x, c, s, y, a, W, kinds = glm_case(rows, D, K)
    ref = glm_eval64(x, c, s, y, a, W, kinds)
    # what the score's error may do to the residual and the row loss, relative to the gradient's and the loss's own scales
    a64, f_abs = a.astype(np.float64), np.abs(ref["grad_scale"])
    u1 = np.concatenate([np.abs((x.astype(np.float64) - c) * s), np.ones((rows, 1))], axis=1)
    kappa_g = float(np.max(((a64[:, None] * ref["score_scale"]).T @ u1) / np.maximum(f_abs, 1e-300)))
    z = ref["scores"]
    logistic = np.array([k == LOGISTIC for k in kinds])
    resid = np.abs(np.where(logistic, U.sigmoid(z) - y, z - y))
    kappa_l = float(np.max((a64[:, None] * ref["score_scale"] * resid).sum(0) / ref["loss_scale"]))
    return ref, kappa_g, kappa_l


@functools.lru_cache(maxsize=None)
def _errors(rows, D, K, layout):
    x, c, s, y, a, W, kinds = glm_case(rows, D, K)
    ref, _, _ = _reference(rows, D, K)
    loss, g, z = _kernels().glm_eval(_layout(x, layout), c, s, y, W, kinds, row_weight=a, scores=True)
    z = z.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss).all() and np.isfinite(g).all() and np.isfinite(z).all()
    return (float(np.max(np.abs(z - ref["scores"]) / ref["score_scale"])), float(np.max(np.abs(g - ref["grad"]) / ref["grad_scale"])),
            float(np.max(np.abs(loss - ref["loss"]) / ref["loss_scale"])))


def _ceilings():
    kg = max(_reference(*shape)[1] for shape in SHAPES)
    kl = max(_reference(*shape)[2] for shape in SHAPES)
    return (GLM_RUN_ROWS + 9) * EPS + SCORE_CEILING * kg, 9 * EPS + SCORE_CEILING * kl


def test_tolerances_are_inside_the_rounding_model():
    grad_ceiling, loss_ceiling = _ceilings()
    print(f"ceilings: scores {SCORE_CEILING:.3e}, gradient {grad_ceiling:.3e}, loss {loss_ceiling:.3e}")
    assert (SCORE_TOL, GRAD_TOL, LOSS_TOL) == (4 * SCORE_OBSERVED, 4 * GRAD_OBSERVED, 4 * LOSS_OBSERVED)
    assert SCORE_TOL <= SCORE_CEILING and GRAD_TOL <= grad_ceiling and LOSS_TOL <= loss_ceiling


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,D,K", SHAPES)
def test_mixed_heads_vs_double(rows, D, K, layout):
    es, eg, el = _errors(rows, D, K, layout)
    print(f"glm_eval {rows}x{D} K={K} {layout}: scores {es:.3e}, gradient {eg:.3e}, loss {el:.3e}; "
          f"asserted {SCORE_TOL:.3e} / {GRAD_TOL:.3e} / {LOSS_TOL:.3e}")
    assert es <= SCORE_TOL and eg <= GRAD_TOL and el <= LOSS_TOL


def test_extreme_logits_and_zero_weights():
    """Scores of +-100 (exp(-100) underflows nothing, exp(100) is never formed) and rows of weight 0, among ordinary rows."""
    rows, D = 64, 6
    rs = np.random.default_rng(3)
    x = rs.standard_normal((rows, D)).astype(np.float32)
    x[:, 0] = np.where(np.arange(rows) % 2 == 0, 1.0, -1.0)
    x[8:, 0] *= 0.01                                              # rows 0 .. 7: z = +-100, the rest ordinary
    W = np.zeros((2, D + 1), dtype=np.float32)
    W[:, 0] = 100.0
    W[:, 1:D] = 0.1 * rs.standard_normal((2, D - 1))
    x[:8, 1:] = 0.0
    y = (rs.random((rows, 2)) < 0.5).astype(np.float32)
    a = np.where(np.arange(rows) % 5 == 0, 0.0, 1.0).astype(np.float32)
    c, s, kinds = np.zeros(D, dtype=np.float32), np.ones(D, dtype=np.float32), [LOGISTIC, SQUARED]
    ref = glm_eval64(x, c, s, y, a, W, kinds)
    assert np.abs(ref["scores"][:8]).min() == 100.0
    loss, g, z = _kernels().glm_eval(_t(x), c, s, y, W, kinds, row_weight=a, scores=True)
    z = z.cpu().numpy().astype(np.float64)
    assert np.isfinite(loss).all() and np.isfinite(g).all() and np.isfinite(z).all()
    es, eg = np.max(np.abs(z - ref["scores"]) / ref["score_scale"]), np.max(np.abs(g - ref["grad"]) / np.maximum(ref["grad_scale"], 1e-300))
    el = np.max(np.abs(loss - ref["loss"]) / ref["loss_scale"])
    print(f"extreme logits: scores {es:.3e}, gradient {eg:.3e}, loss {el:.3e}")
    assert es <= SCORE_TOL and eg <= GRAD_TOL and el <= LOSS_TOL
    # weight-0 rows alone: nothing but zeros
    loss0, g0, _ = _kernels().glm_eval(_t(x), c, s, y, W, kinds, row_weight=np.zeros(rows, dtype=np.float32))
    assert not loss0.any() and not g0.any()


# ---- 3. empty outputs, dropped columns, same bits, additivity ---------------------------------------------------------------------
@pytest.mark.parametrize("rows,D,K", [SHAPES[2], SHAPES[4], SHAPES[5]])
def test_empty_outputs_dropped_columns_and_same_bits(rows, D, K):
    x, c, s, y, a, W, kinds = glm_case(rows, D, K)
    s = s.copy()
    s[::3] = 0.0                                                  # every third column dropped
    t, k = _t(x), _kernels()
    loss, g, z = k.glm_eval(t, c, s, y, W, kinds, row_weight=a, scores=True)
    loss2, g2, z2 = k.glm_eval(t, c, s, y, W, kinds, row_weight=a, scores=True)
    assert np.array_equal(loss.view(np.int64), loss2.view(np.int64)) and np.array_equal(g.view(np.int64), g2.view(np.int64))
    assert torch.equal(z.view(torch.int32), z2.view(torch.int32))
    _, none, z_only = k.glm_eval(t, c, s, y, W, kinds, row_weight=a, grad=False, scores=True)
    assert none is None and torch.equal(z.view(torch.int32), z_only.view(torch.int32))      # the predictor: the full call's bits
    _, _, z_blind = k.glm_eval(t, c, s, None, W, kinds, grad=False, scores=True)             # ... without targets too
    assert torch.equal(z.view(torch.int32), z_blind.view(torch.int32))
    loss3, g3, no_scores = k.glm_eval(t, c, s, y, W, kinds, row_weight=a)
    assert no_scores is None and np.array_equal(g.view(np.int64), g3.view(np.int64)) and np.array_equal(loss.view(np.int64), loss3.view(np.int64))
    assert not g[:, :D][:, ::3].any() and g[:, :D][:, 1::3].all()
    ref = glm_eval64(x, c, s, y, a, W, kinds)
    live = ref["grad_scale"] > 0
    assert np.max(np.abs(g - ref["grad"])[live] / ref["grad_scale"][live]) <= GRAD_TOL


@pytest.mark.parametrize("rows,D,K", SHAPES[2:5])
def test_row_halves_add_up(rows, D, K):
    x, c, s, y, a, W, kinds = glm_case(rows, D, K)
    ref, _, _ = _reference(rows, D, K)
    h = rows // 2 + 1
    t, k = _t(x), _kernels()
    parts = [k.glm_eval(t[lo:hi], c, s, y[lo:hi], W, kinds, row_weight=a[lo:hi]) for lo, hi in ((0, h), (h, rows))]
    loss, g = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert np.max(np.abs(g - ref["grad"]) / ref["grad_scale"]) <= GRAD_TOL and np.max(np.abs(loss - ref["loss"]) / ref["loss_scale"]) <= LOSS_TOL
    # and through the host's own adder, as the two cohorts of the classifier two-sample test
    one = ShardComm(False)
    loss_p, g_p = glm_sums(k, [(one, t[:h], _t(y[:h]), _t(a[:h])), (one, t[h:], _t(y[h:]), _t(a[h:]))], c, s, W, list(kinds))
    assert np.array_equal(loss_p, loss) and np.array_equal(g_p, g)


def test_column_moments_vs_double():
    x = glm_case(1000, 258, 4)[0]
    c = x.astype(np.float64).mean(0).astype(np.float32)
    d = x.astype(np.float64) - c.astype(np.float64)
    for layout in LAYOUTS:
        s, q = _kernels().col_centered_moments(_layout(x, layout), c)
        s2, q2 = _kernels().col_centered_moments(_layout(x, layout), c)
        assert np.array_equal(s.view(np.int64), s2.view(np.int64)) and np.array_equal(q.view(np.int64), q2.view(np.int64))
        assert np.max(np.abs(s - d.sum(0)) / np.abs(d).sum(0)) <= 1e-13 and np.max(np.abs(q / (d * d).sum(0) - 1.0)) <= 1e-13
    s0, q0 = _kernels().col_centered_moments(_t(x))
    assert np.allclose(s0, x.astype(np.float64).sum(0), rtol=1e-13) and np.allclose(q0, (x.astype(np.float64) ** 2).sum(0), rtol=1e-13)


def test_argument_errors():
    k = _kernels()
    x = torch.zeros((4, 3), device="cuda")
    ok = dict(center=np.zeros(3), scale=np.ones(3), y=np.zeros((4, 1)), W=np.zeros((1, 4)), kinds=[LOGISTIC])
    with pytest.raises(ValueError):
        k.glm_eval(x, ok["center"], ok["scale"], np.zeros((4, 5)), np.zeros((5, 4)), [LOGISTIC] * 5)            # K > 4
    with pytest.raises(ValueError):
        k.glm_eval(x, ok["center"], ok["scale"], ok["y"], ok["W"], [7])                                         # unknown kind
    with pytest.raises(ValueError):
        k.glm_eval(x, ok["center"], ok["scale"], None, ok["W"], [LOGISTIC])                                     # a gradient without targets
    with pytest.raises(ValueError):
        k.glm_eval(torch.zeros((2, 8193), device="cuda"), np.zeros(8193), np.ones(8193), np.zeros((2, 1)), np.zeros((1, 8194)), [SQUARED])
    lib, stream = L.lib(), C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    kind = (C_.c_int32 * 1)(0)
    out = (C_.c_double * 1)()
    args = lambda rows, ld, D, K: (stream, 0, L.ptr(x), rows, ld, D, L.ptr(x), L.ptr(x), L.ptr(x), 1, None, L.ptr(x), K, kind, out, None, None, 0)
    for rows, ld, D, K in ((0, 3, 3, 1), (4, 2, 3, 1), (4, 3, 0, 1), (4, 3, 3, 0), (4, 3, 3, 5)):
        assert lib.osd_val_glm_eval(*args(rows, ld, D, K)) == L.OSD_EINVAL


# ---- 4. fits ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_fit():
    x, c, s, y, a, _, kinds = glm_case(257, 130, 3)
    k, one, t = _kernels(), ShardComm(False), _t(x)
    n, l2 = float(a.astype(np.float64).sum()), 1e-2
    parts = [(one, t, _t(y), _t(a))]
    fit = U.fit_glm(lambda W: glm_sums(k, parts, c, s, W, list(kinds)), 3, 130, list(kinds), n, l2)
    g = penalised_gradient64(x, c, s, y, a, fit["W"], kinds, n, l2)
    return fit, float(np.abs(g).max())


def test_device_fit_reaches_the_optimum():
    fit, gnorm = _device_fit()
    print(f"device fit: {fit['iterations']} iterations, converged {fit['converged']}, device |g|_inf {fit['grad_inf_norm']:.3e}, "
          f"float64 |g|_inf at its W {gnorm:.3e}; asserted {4 * FIT_OBSERVED:.3e}")
    assert np.isfinite(fit["W"]).all() and fit["iterations"] >= 5
    assert gnorm <= 4 * FIT_OBSERVED                              # |W - W*| <= gnorm / l2: strongly convex


# ---- 5. end to end on planted cohorts ------------------------------------------------------------------------------------------------
NAMES = ["event", "time"]


def _cohorts():
    (train, train_cond), (synth, cond), (test, test_cond) = planted(seed=3), planted(seed=4), planted(seed=5)
    return train, train_cond, synth, cond, test, test_cond


@functools.lru_cache(maxsize=None)
def _utility_both(permuted):
    train, train_cond, synth, cond, test, test_cond = _cohorts()
    if permuted:
        cond = cond[np.random.default_rng(11).permutation(len(cond))]
    dev = BiologicalValidator(CONF).downstream_utility(train, train_cond, synth, cond, test, test_cond, names=NAMES)
    t = lambda a: torch.from_numpy(np.array(a))
    ref = utility_metrics(ShardComm(False), NumpyKernels(), t(train), train_cond, t(synth), cond, t(test), test_cond, NAMES)
    return dev, ref


@functools.lru_cache(maxsize=None)
def _c2st_both(shifted):
    (sa, sb), split = C2ST_SEEDS
    real, synth = planted(seed=sa)[0], planted(seed=sb, shift_col=9 if shifted else None)[0]
    dev = BiologicalValidator(CONF).discriminator_test(real, synth, seed=split)
    t = lambda a: torch.from_numpy(np.array(a))
    return dev, c2st_metrics(ShardComm(False), NumpyKernels(), t(real), t(synth), seed=split)


@pytest.mark.parametrize("permuted", [False, True])
def test_downstream_utility_vs_float64_pipeline(permuted):
    dev, ref = _utility_both(permuted)
    assert set(dev) == set(ref) == {"utility_tstr_auc_event", "utility_trtr_auc_event", "utility_auc_gap_event", "utility_tstr_r2_time",
                                    "utility_trtr_r2_time", "utility_r2_gap_time", "utility_gap_mean"}
    worst = max(abs(dev[key] - ref[key]) for key in ref)
    print(f"downstream_utility permuted={permuted}: max |device - float64| = {worst:.3e}; asserted {4 * E2E_OBSERVED:.3e}", dev)
    assert worst <= 4 * E2E_OBSERVED


def test_permuted_conditions_lose_the_utility_and_nothing_else():
    """The demonstration behind the feature: the same synthetic rows with permuted conditions keep every feature-only figure and
    lose the downstream utility; the faithful cohort trains a predictor as good as real patients do."""
    (good, good64), (bad, bad64) = _utility_both(False), _utility_both(True)
    assert good64["utility_tstr_auc_event"] > 0.8 and bad64["utility_tstr_auc_event"] < 0.6      # the float64 pipeline alone
    assert good["utility_tstr_auc_event"] > 0.8 and bad["utility_tstr_auc_event"] < 0.6
    assert abs(good["utility_auc_gap_event"]) < 0.05 and bad["utility_auc_gap_event"] > 0.25
    assert good["utility_tstr_r2_time"] > 0.5 and bad["utility_tstr_r2_time"] < 0.1
    # the feature matrix is the same array in both runs, so every figure that reads features alone is the same by construction;
    # so is everything trained on real patients
    assert good["utility_trtr_auc_event"] == bad["utility_trtr_auc_event"] and good["utility_trtr_r2_time"] == bad["utility_trtr_r2_time"]


def test_discriminator_vs_float64_pipeline():
    for shifted in (False, True):
        dev, ref = _c2st_both(shifted)
        assert set(dev) == set(ref) == {"c2st_auc", "c2st_accuracy", "c2st_pmse"}
        worst = max(abs(dev[key] - ref[key]) for key in ("c2st_auc", "c2st_pmse"))
        print(f"discriminator_test shifted={shifted}: max |device - float64| = {worst:.3e}; asserted {4 * E2E_OBSERVED:.3e}", dev)
        assert worst <= 4 * E2E_OBSERVED
    same, shifted = _c2st_both(False)[0], _c2st_both(True)[0]
    assert _c2st_both(True)[1]["c2st_auc"] > 0.9 and shifted["c2st_auc"] > 0.9 and shifted["c2st_pmse"] > same["c2st_pmse"]
    assert abs(same["c2st_auc"] - 0.5) < 0.1 and same["c2st_pmse"] < 0.1


def test_validate_all_adds_the_keys_only_when_asked():
    import pandas as pd
    def frames(n, seed):
        x, cond = planted(n=n, D=52, seed=seed)
        m = pd.DataFrame((x[:, :20] > 0).astype(np.float32), columns=[f"M{i}" for i in range(20)])
        e = pd.DataFrame(x[:, 20:50], columns=[f"G{i}" for i in range(30)])
        p = pd.DataFrame(x[:, 50:52], columns=["PW0", "PW1"])
        return m, e, p, cond
    rm, re_, rp, rc = frames(200, 3)
    sm, se, sp, sc = frames(240, 4)
    tm, te, tp, tc = frames(150, 5)
    val = BiologicalValidator(CONF)
    np.random.seed(0)
    plain = val.validate_all(rm, re_, rp, sm, se, sp)
    np.random.seed(0)
    full = val.validate_all(rm, re_, rp, sm, se, sp, utility=(rc, sc, (tm, te, tp), tc), c2st=True)
    extra = set(full) - set(plain)
    assert extra == {"utility_tstr_auc_c0", "utility_trtr_auc_c0", "utility_auc_gap_c0", "utility_tstr_r2_c1", "utility_trtr_r2_c1",
                     "utility_r2_gap_c1", "utility_gap_mean", "c2st_auc", "c2st_accuracy", "c2st_pmse"}
    assert all(abs(full[key] - plain[key]) <= 1e-9 * max(1.0, abs(plain[key])) for key in plain)      # (the MMD's double atomics: last bits)
    assert all(np.isfinite(full[key]) for key in extra)


# ---- 6. sharded -----------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    import torch.distributed as dist
    from osteosarcoma_diffusionmodel_amd.parallel import shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        train, train_cond, synth, cond, test, test_cond = _cohorts()
        off, cnt = shard_rows(len(synth), rank, world)
        val = BiologicalValidator(CONF, sharded=True)
        assert val.comm.on
        res = val.downstream_utility(train, train_cond, synth[off:off + cnt], cond[off:off + cnt], test, test_cond, names=NAMES)
        (sa, sb), split = C2ST_SEEDS
        shifted = planted(seed=sb, shift_col=9)[0]
        res.update(val.discriminator_test(planted(seed=sa)[0], shifted[off:off + cnt], seed=split))
        q.put((rank, res))
    except Exception as e:
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_validator_reports_the_unsharded_figures():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    assert all(isinstance(r[1], dict) for r in res), res
    ref = dict(_utility_both(False)[0])
    ref.update(_c2st_both(True)[0])
    for _, r in res:
        assert set(r) == set(ref)
        worst = max(abs(r[key] - ref[key]) for key in ref)
        print(f"sharded against unsharded: max difference {worst:.3e}; asserted {4 * E2E_OBSERVED:.3e}")
        assert worst <= 4 * E2E_OBSERVED
    assert res[0][1] == res[1][1]                    # identical numbers on every rank
