"""GPU: the label-sum kernel (osd_val_label_sums: label_sums_kernel + label_sums_reduce, csrc/cluster.hip), ``cluster.kmeans`` on the
device kernels and ``BiologicalValidator.subtype_fidelity`` above them, against the float64 restatement of tests/cluster_helpers.py
evaluated on the same fp32 inputs.

label_sums shapes (rows, D, K): (1, 5, 1), (33, 6, 2), (257, 130, 3), (1000, 258, 4), (515, 5142, 5), (100001, 8, 7), (4099, 64, 64)
-- one row; row tails (a register set is 8 rows); D below one wavefront; D % 4 == 2; the reference's width (21 column blocks, the
last one with 22 live lanes); many row blocks with a ragged last one (256 blocks of 391 rows, the last of 296); the largest K (two
wavefronts per workgroup, 1024 rows per block).  Each runs dense, as an aligned and as an unaligned column slice of a wider matrix
full of 1000s.  Labels are random with some -1 and some K mixed in and one cluster left empty.

  * integers (|x| < 2^12): sums, counts and value sums must EQUAL the int64 result;
  * real data: every sum within rows x 2^-52 x sum |x| of float64 NumPy -- double adds, reordered, can do no worse;
  * two calls return identical bits; bad arguments return OSD_EINVAL.

One Lloyd step and whole fits: the device's labels may differ from the float64 labels only on AMBIGUOUS rows, whose float64 margin
d2_(2) - d2_(1) is below 2 (D + 4) 2^-24 (|x|^2 + max |c|^2), the worst case of the fp32 expanded form the Gram pass ranks by; the
whole fits first assert that the reference's margin is at least 8 x that bound at every pass, and then demand equal labels and
iteration counts.  New centroids against float64 centroids from the device's own labels: 2^-24 max(|C|, 1e-30) per entry (one fp32
rounding of the quotient) plus the sum bound above over the count.  Inertia against the float64 inertia at the device's labels and
centroids: k_knn_refine rounds each difference to fp32 (2 x 2^-24 on its square), sums in double (D x 2^-52) and rounds the row's
distance to fp32 (2^-24).

End to end (600 real, 900 synthetic, D = 130, K = 4): counts and shares are exact; the ratios, shifts and the inertia are held to
the float64 pipeline (the validator's own host code over the float64 kernels) relative to max(1, |value|).
    Measured, the largest over the real-valued keys: faithful 3.222e-9, one subtype removed 4.991e-9, one subtype collapsed 3.771e-9,
    condition inverted 4.274e-9 -- the fp32 rounding of the recomputed distances, averaged over a subtype's rows.  Asserted: 4 x
    the largest.  In the same run: no device label differed from float64 in the three Lloyd steps (0, 22 and 6 ambiguous rows), the
    new centroids came within 0.94 - 0.99 of their tolerance (the fp32 rounding of the quotient is the whole of it), and the sums on
    real data equalled NumPy's (fp32 values of one magnitude add exactly in double)."""
import ctypes as C_
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import cluster as CL
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels, subtype_summary
from cluster_helpers import EPS, NumpyKernels, ambiguity_bound, blobs, centred, label_sums64, margins

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 1), (33, 6, 2), (257, 130, 3), (1000, 258, 4), (515, 5142, 5), (100001, 8, 7), (4099, 64, 64)]
LAYOUTS = ["dense", "slice_aligned", "slice_unaligned"]
U53 = 2.0 ** -52
E2E_OBSERVED = 4.991e-9           # measured max |device - float64| / max(1, |float64|) over the real-valued keys of the four samplers
E2E_TOL = 4 * E2E_OBSERVED
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


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _labels(rows, K):
    """int32 [rows]: random labels, about a tenth of them outside [0, K) (-1 and K), and -- from K = 2 -- cluster K // 2 left empty."""
    rs = np.random.default_rng(977 * rows + K)
    lab = rs.integers(0, K, rows)
    if K >= 2:
        lab[lab == K // 2] = (K // 2 + 1) % K
    u = rs.random(rows)
    lab[u < 0.05] = -1
    lab[u > 0.95] = K
    return lab.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _int_case(rows, D, K):
    rs = np.random.default_rng(131 * rows + 7 * D + K)
    x = rs.integers(-4095, 4096, (rows, D))
    v = rs.integers(0, 4096, rows)
    lab = _labels(rows, K)
    sums, counts, vs = np.zeros((K, D), dtype=np.int64), np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    for k in range(K):
        sel = lab == k
        sums[k], counts[k], vs[k] = x[sel].sum(0), sel.sum(), v[sel].sum()
    return x.astype(np.float32), v.astype(np.float32), lab, sums, counts, vs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,D,K", SHAPES)
def test_label_sums_exact_on_integers(rows, D, K, layout):
    x, v, lab, sums, counts, vs = _int_case(rows, D, K)
    s, c, w = _kernels().label_sums(_layout(x, layout), _t(lab), K, value=_t(v))
    assert s.dtype == torch.float64 and tuple(s.shape) == (K, D) and c.dtype == torch.int64 and tuple(c.shape) == (K,)
    assert w.dtype == torch.float64 and tuple(w.shape) == (K,)
    if K >= 2:
        assert counts[K // 2] == 0 and counts.sum() < rows       # an empty cluster, and rows that belong to none
    assert np.array_equal(c.cpu().numpy(), counts)
    got = s.cpu().numpy()
    assert np.array_equal(got, sums.astype(np.float64)), f"{int((got != sums).sum())} of {got.size} sums differ"
    assert np.array_equal(w.cpu().numpy(), vs.astype(np.float64))
    s2, c2, none = _kernels().label_sums(_layout(x, layout), _t(lab), K)      # without a value
    assert none is None and torch.equal(s2, s) and torch.equal(c2, c)


@functools.lru_cache(maxsize=None)
def _real_case(rows, D, K):
    rs = np.random.default_rng(7919 * rows + 31 * D + K)
    x = (rs.standard_normal((rows, D)) * (0.5 + rs.random(D)) + 3.0 * rs.standard_normal(D)).astype(np.float32)
    v = (rs.random(rows) * 50.0).astype(np.float32)
    lab = _labels(rows, K)
    sums, counts, vs = label_sums64(x, lab, K, v)
    bound = rows * U53 * label_sums64(np.abs(x), lab, K)[0]
    return x, v, lab, sums, counts, vs, bound, rows * U53 * vs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,D,K", SHAPES)
def test_label_sums_against_float64(rows, D, K, layout):
    x, v, lab, sums, counts, vs, bound, vbound = _real_case(rows, D, K)
    xt, lt, vt = _layout(x, layout), _t(lab), _t(v)
    s, c, w = _kernels().label_sums(xt, lt, K, value=vt)
    got = s.cpu().numpy()
    err = np.abs(got - sums)
    print(f"label_sums {rows}x{D} K={K} {layout}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert np.isfinite(got).all() and np.array_equal(c.cpu().numpy(), counts)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (np.abs(w.cpu().numpy() - vs) <= vbound).all()
    s2, c2, w2 = _kernels().label_sums(xt, lt, K, value=vt)                   # the same inputs: the same bits
    assert torch.equal(s2, s) and torch.equal(c2, c) and torch.equal(w2, w)


def test_label_sums_every_row_in_one_cluster():
    x, v, _, _, _, _ = _int_case(1000, 258, 4)
    lab = np.full(1000, 2, dtype=np.int32)
    s, c, w = _kernels().label_sums(_t(x), _t(lab), 4, value=_t(v))
    want = np.zeros((4, 258))
    want[2] = x.astype(np.int64).sum(0)
    assert np.array_equal(s.cpu().numpy(), want) and c.cpu().tolist() == [0, 0, 1000, 0]
    assert w.cpu().tolist() == [0.0, 0.0, float(v.astype(np.int64).sum()), 0.0]
    # labels that belong to no cluster at all: nearest's -1
    s, c, _ = _kernels().label_sums(_t(x), _t(np.full(1000, -1, dtype=np.int32)), 4)
    assert not s.any().item() and not c.any().item()


def test_label_sums_argument_errors():
    lib = L.lib()
    x = torch.zeros((8, 8), device="cuda")
    lab = torch.zeros(8, dtype=torch.int32, device="cuda")
    val = torch.zeros(8, device="cuda")
    sums = torch.zeros((64, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int64, device="cuda")
    vs = torch.zeros(64, dtype=torch.float64, device="cuda")
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(rows=8, ld=8, D=8, K=2, x=x, lab=lab, value=None, sums=sums, cnt=cnt, vs=None):
        return lib.osd_val_label_sums(stream, 0, L.ptr(x), rows, ld, D, L.ptr(lab), K, L.ptr(value), L.ptr(sums), L.ptr(cnt), L.ptr(vs))

    assert call() == L.OSD_OK and call(value=val, vs=vs) == L.OSD_OK and call(K=64) == L.OSD_OK
    for bad in (dict(rows=0), dict(D=0), dict(D=8193, ld=8193), dict(ld=7), dict(K=0), dict(K=65), dict(K=-1), dict(x=None), dict(lab=None),
                dict(sums=None), dict(cnt=None), dict(value=val), dict(vs=vs)):
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error()
    k = _kernels()
    with pytest.raises(ValueError):
        k.label_sums(x, lab, 65)
    with pytest.raises(ValueError):
        k.label_sums(x, lab[:7], 2)
    with pytest.raises(ValueError):
        k.label_sums(x, lab, 2, value=val[:7])


# ---- 2. one Lloyd step on overlapping blobs ---------------------------------------------------------------------------------------
class Recorder:
    """DeviceKernels that keeps every ``nearest`` result: what the host code saw, pass by pass."""

    def __init__(self):
        self.k = _kernels()
        self.passes = []

    def nearest(self, q, r, exclude=None):
        d2, idx = self.k.nearest(q, r, exclude)
        self.passes.append((r.clone(), d2, idx))
        return d2, idx

    def label_sums(self, t, labels, K, value=None):
        return self.k.label_sums(t, labels, K, value=value)


def _centroid_check(x, labels, K, got, what):
    """The centroids of the device's own labels: float64 means, one fp32 rounding of the quotient, and the sum bound over the count."""
    sums, counts, _ = label_sums64(x, labels, K)
    assert (counts > 0).all(), what
    mean = sums / counts[:, None]
    tol = EPS * np.maximum(np.abs(mean), 1e-30) + x.shape[0] * U53 * label_sums64(np.abs(x), labels, K)[0] / counts[:, None]
    err = np.abs(got.astype(np.float64) - mean)
    print(f"{what}: centroid err / tol {float((err / tol).max()):.3g}")
    assert (err <= tol).all(), (what, float((err / tol).max()))


STEP_CASES = [(1000, 130, 4, 0.25), (515, 5142, 5, 0.05), (4099, 258, 16, 0.2)]


@functools.lru_cache(maxsize=None)
def _step_case(n, D, K, sep):
    x = centred(blobs(n, D, K, sep)[0])
    rows = np.random.default_rng(n + D + K).choice(n, size=K, replace=False)
    c = np.array(x[rows])
    labels, d2, margin = margins(x, c)
    return x, c, labels, margin < ambiguity_bound(x, c)


@pytest.mark.parametrize("n,D,K,sep", STEP_CASES)
def test_one_lloyd_step(n, D, K, sep):
    x, c, labels64, ambiguous = _step_case(n, D, K, sep)
    share = float(ambiguous.mean())
    print(f"lloyd step {n}x{D} K={K} sep={sep}: ambiguous share {share:.4f}")
    assert share <= 0.10
    rec = Recorder()
    fit = CL.lloyd(_t(x), _t(c), 2, rec)                      # assign, update, assign
    assert len(rec.passes) == 2 and fit.iterations == 2
    labels = rec.passes[0][2].cpu().numpy().astype(np.int64)
    differ = labels != labels64
    print(f"  device labels differ on {int(differ.sum())} rows, {int(ambiguous.sum())} ambiguous")
    assert not (differ & ~ambiguous).any() and labels.min() >= 0 and labels.max() < K
    assert torch.equal(rec.passes[1][0], fit.centroids)
    _centroid_check(x, labels, K, fit.centroids.cpu().numpy(), f"step {n}x{D}")


# ---- 3. whole fits ----------------------------------------------------------------------------------------------------------------
FIT_CASES = [(37, 5, 2, 3.0), (300, 6, 3, 4.0), (1000, 130, 4, 2.0), (515, 5142, 5, 0.5), (4099, 258, 16, 1.0), (20001, 8, 7, 6.0)]
LONG_SEED = 8                     # the init rows of the long trajectory (chosen on the CPU: see test_long_trajectory)


@functools.lru_cache(maxsize=None)
def _fit_reference(n, D, K, sep, init_seed=None):
    x = centred(blobs(n, D, K, sep)[0])
    if init_seed is None:
        init = np.array(x[:K])                                 # the first row of each true blob
    else:
        init = np.array(x[np.random.default_rng(init_seed).choice(n, size=K, replace=False)])
    nk = NumpyKernels()
    ref = CL.kmeans(torch.from_numpy(x), K, init=init, kernels=nk)
    return x, init, ref, nk.min_ratio


def _fit_check(n, D, K, sep, init_seed=None):
    x, init, ref, ratio = _fit_reference(n, D, K, sep, init_seed)
    print(f"fit {n}x{D} K={K} sep={sep}: {ref.iterations} passes, smallest margin {ratio:.3g} x the ambiguity bound")
    assert ref.converged and ratio >= 8.0                      # the precondition: no pass of the reference has an ambiguous row
    fit = CL.kmeans(_t(x), K, init=init, kernels=_kernels())
    assert fit.converged and fit.iterations == ref.iterations
    assert torch.equal(fit.labels.cpu(), ref.labels) and np.array_equal(fit.counts, ref.counts) and fit.empty == ref.empty
    labels = fit.labels.cpu().numpy().astype(np.int64)
    c = fit.centroids.cpu().numpy()
    _centroid_check(x, labels, K, c, f"fit {n}x{D}")
    d2 = ((x.astype(np.float64) - c.astype(np.float64)[labels]) ** 2).sum(1)
    tol = (3 * EPS + D * U53) * d2
    err = np.abs(fit.d2.cpu().numpy().astype(np.float64) - d2)
    assert (err <= tol).all()
    print(f"  inertia {fit.inertia:.9g} against {float(d2.sum()):.9g}, err / tol {abs(fit.inertia - d2.sum()) / tol.sum():.3g}")
    assert abs(fit.inertia - float(d2.sum())) <= float(tol.sum())
    return ref


@pytest.mark.parametrize("n,D,K,sep", FIT_CASES)
def test_whole_fit_equals_float64(n, D, K, sep):
    _fit_check(n, D, K, sep)


def test_long_trajectory():
    """300 x 6, K = 3, sep 1.5, init K random rows: many reassigning passes, every one with all margins at least 8 x the bound.  Of
    the init seeds 0 .. 39 run through the float64 reference on the CPU, seeds 8 and 20 give the longest fits that pass the 8 x
    precondition: 16 passes, at a smallest margin of 361 x (seed 8) and 69 x the bound."""
    ref = _fit_check(300, 6, 3, 1.5, init_seed=LONG_SEED)
    assert ref.iterations == 16


# ---- 4. subtype_fidelity end to end -----------------------------------------------------------------------------------------------
N_REAL, N_SYNTH, E2E_D, E2E_K = 600, 900, 130, 4


@functools.lru_cache(maxsize=None)
def _mixture():
    rs = np.random.default_rng(20)
    return 3.0 * rs.standard_normal((E2E_K, E2E_D)), np.array([0.4, 0.3, 0.2, 0.1])      # centres far enough apart for k-means++ to find each


def _draw(n, seed, weights=None, noise=None):
    """(x float32 [n, D], truth, binary condition float32 [n, 1]) from the planted mixture; ``noise``: per-subtype noise scale."""
    mu, w = _mixture()
    w = w if weights is None else np.asarray(weights, dtype=np.float64)
    rs = np.random.default_rng(seed)
    truth = rs.choice(E2E_K, size=n, p=w / w.sum())
    scale = np.ones(E2E_K) if noise is None else np.asarray(noise, dtype=np.float64)
    x = mu[truth] + scale[truth][:, None] * rs.standard_normal((n, E2E_D))
    cond = (rs.random(n) < 0.2 + 0.15 * truth).astype(np.float32)
    return x.astype(np.float32), truth, cond[:, None]


@functools.lru_cache(maxsize=None)
def _samplers():
    real = _draw(N_REAL, 1)
    faithful = _draw(N_SYNTH, 2)
    removed = _draw(N_SYNTH, 3, weights=[0.4, 0.3, 0.0, 0.1])
    collapsed = _draw(N_SYNTH, 4, noise=[1.0, 0.3, 1.0, 1.0])
    x, truth, cond = _draw(N_SYNTH, 5)
    inverted = (x, truth, np.where(truth[:, None] == 0, 1.0 - cond, cond).astype(np.float32))
    return real, {"faithful": faithful, "removed": removed, "collapsed": collapsed, "inverted": inverted}


@functools.lru_cache(maxsize=None)
def _pipeline64(name):
    """The float64 pipeline: the validator's own host code over the float64 kernels."""
    real, samplers = _samplers()
    s = samplers[name]
    rows = CL.subtype_rows(ShardComm(False), NumpyKernels(), torch.from_numpy(real[0]), torch.from_numpy(s[0]), E2E_K,
                           conditions=(torch.from_numpy(real[2]), torch.from_numpy(s[2])), names=["met"], seed=0, n_init=4)
    return subtype_summary(rows), rows


@functools.lru_cache(maxsize=None)
def _device(name):
    real, samplers = _samplers()
    s = samplers[name]
    return BiologicalValidator(CONF).subtype_fidelity(real[0], s[0], E2E_K, conditions=(real[2], s[2]), names=["met"], return_rows=True)


EXACT_KEYS = ("subtype_k", "subtype_iterations", "subtype_converged", "subtype_missing", "subtype_min_share_ratio", "subtype_tv_distance",
              "subtype_js_divergence", "subtype_condition_gap_met")


def _compare(got, want, tol):
    assert list(got) == list(want)
    worst = 0.0
    for key, w in want.items():
        g = got[key]
        if key in EXACT_KEYS or "_share_" in key:              # functions of the counts (and of exact 0/1 sums) alone
            assert g == w or (np.isnan(g) and np.isnan(w)), (key, g, w)
        elif np.isnan(w):
            assert np.isnan(g), (key, g, w)
        else:
            worst = max(worst, abs(g - w) / max(1.0, abs(w)))
            assert abs(g - w) <= tol * max(1.0, abs(w)), (key, g, w)
    return worst


@pytest.mark.parametrize("name", ["faithful", "removed", "collapsed", "inverted"])
def test_subtype_fidelity_equals_float64_pipeline(name):
    (got, rows), (want, rows64) = _device(name), _pipeline64(name)
    assert np.array_equal(rows["real_counts"], rows64["real_counts"]) and np.array_equal(rows["synth_counts"], rows64["synth_counts"])
    assert np.array_equal(rows["real_labels"], rows64["real_labels"]) and np.array_equal(rows["synth_labels"], rows64["synth_labels"])
    assert rows["real_counts"].tolist() == sorted(rows["real_counts"].tolist(), reverse=True) and rows["real_counts"].sum() == N_REAL
    assert rows["centroids"].shape == (E2E_K, E2E_D) and rows["real_d2"].shape == (N_REAL,) and rows["synth_d2"].shape == (N_SYNTH,)
    worst = _compare(got, want, E2E_TOL)
    print(f"subtype_fidelity {name}: largest |device - float64| / max(1, |float64|) = {worst:.3e}")


def test_subtype_fidelity_faithful_sampler():
    got, want = _device("faithful")[0], _pipeline64("faithful")[0]
    # two real halves drawn from the same mixture, by the float64 pipeline: what sampling noise alone gives at 300 rows
    a, b = _draw(N_REAL // 2, 11), _draw(N_REAL // 2, 12)
    halves = subtype_summary(CL.subtype_rows(ShardComm(False), NumpyKernels(), torch.from_numpy(a[0]), torch.from_numpy(b[0]), E2E_K,
                                             seed=0, n_init=4))
    print(f"faithful: JS {got['subtype_js_divergence']:.3e}, two real halves {halves['subtype_js_divergence']:.3e}")
    assert got["subtype_js_divergence"] < halves["subtype_js_divergence"]
    assert got["subtype_missing"] == 0 and got["subtype_converged"]
    for k in range(E2E_K):
        assert abs(got[f"subtype_dispersion_ratio_{k}"] - want[f"subtype_dispersion_ratio_{k}"]) <= E2E_TOL * max(1.0, want[f"subtype_dispersion_ratio_{k}"])
        assert 0.9 < got[f"subtype_dispersion_ratio_{k}"] < 1.1


def test_subtype_fidelity_removed_subtype():
    got, rows = _device("removed")
    assert got["subtype_missing"] == 1 and got["subtype_min_share_ratio"] == 0.0
    assert rows["synth_counts"][2] == 0 and np.isnan(got["subtype_dispersion_ratio_2"])      # true weights 0.4 0.3 0.2 0.1: subtype 2


def test_subtype_fidelity_collapsed_subtype():
    """One subtype's noise scaled by 0.3: its dispersion ratio is 0.09 up to sampling.  With n_k real and m_k synthetic rows of the
    subtype, the synthetic mean d2 is 0.09 chi2_D / m_k-averaged plus |centroid - mu|^2 (expectation D / n_k, the centroid is a mean
    of n_k rows), and the real one is chi2_D (1 - 1 / n_k): the ratio is expected at (0.09 D + D / n_k) / (D (1 - 1 / n_k)), both
    chi-square averages having a relative sd of sqrt(2 / (D rows)); the float64 pipeline's value must lie within six such sds, and
    the device's at the float64 pipeline's value."""
    (got, rows), (want, _) = _device("collapsed"), _pipeline64("collapsed")
    k = 1
    n_k, m_k = int(rows["real_counts"][k]), int(rows["synth_counts"][k])
    expected = (0.09 * E2E_D + E2E_D / n_k) / (E2E_D * (1.0 - 1.0 / n_k))
    sd = expected * (np.sqrt(2.0 / (E2E_D * m_k)) + np.sqrt(2.0 / (E2E_D * n_k)) + np.sqrt(2.0 / n_k) * (1.0 / n_k) / 0.09)
    value = want[f"subtype_dispersion_ratio_{k}"]
    print(f"collapsed: ratio {got[f'subtype_dispersion_ratio_{k}']:.6f}, float64 {value:.6f}, expected {expected:.6f} +- {sd:.2e}")
    assert abs(value - expected) <= 6 * sd and 0.09 < value < 0.11
    assert abs(got[f"subtype_dispersion_ratio_{k}"] - value) <= E2E_TOL
    assert got["subtype_dispersion_ratio_min"] == got[f"subtype_dispersion_ratio_{k}"]
    assert all(0.9 < got[f"subtype_dispersion_ratio_{j}"] < 1.1 for j in range(E2E_K) if j != k)


def test_subtype_fidelity_inverted_condition():
    (got, rows), (want, _) = _device("inverted"), _pipeline64("inverted")
    real, samplers = _samplers()
    assert got["subtype_condition_gap_met"] == want["subtype_condition_gap_met"]
    r0 = real[2][rows["real_labels"] == 0, 0].astype(np.float64).mean()
    s0 = samplers["inverted"][2][rows["synth_labels"] == 0, 0].astype(np.float64).mean()
    assert got["subtype_condition_gap_met"] == pytest.approx(abs(r0 - s0), rel=1e-12) and got["subtype_condition_gap_met"] > 0.4
    assert _device("faithful")[0]["subtype_condition_gap_met"] < 0.3      # sampling noise alone: 0.08 sd in the smallest subtype


def test_subtype_fidelity_argument_errors():
    real, samplers = _samplers()
    val = BiologicalValidator(CONF)
    x, y = real[0], samplers["faithful"][0]
    bad = np.array(x)
    bad[3, 7] = np.nan
    for args, kw in (((bad, y, 4), {}), ((x, bad[:, :], 4), {}), ((x[:3], y, 4), {}), ((x, y, 0), {}), ((x, y, 65), {}), ((x, y[:, :100], 4), {}),
                     ((x, y, 4), dict(conditions=(real[2][:-1], samplers["faithful"][2]))),
                     ((x, y, 4), dict(conditions=(real[2], samplers["faithful"][2][:-1]))),
                     ((x, y, 4), dict(conditions=(real[2], samplers["faithful"][2]), names=["a", "b"]))):
        with pytest.raises(ValueError):
            val.subtype_fidelity(*args, **kw)


# ---- 5. row shards ----------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    import torch.distributed as dist
    from osteosarcoma_diffusionmodel_amd.parallel import shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        real, samplers = _samplers()
        s = samplers["inverted"]
        off, cnt = shard_rows(N_SYNTH, rank, world)
        val = BiologicalValidator(CONF, sharded=True)
        assert val.comm.on
        res = val.subtype_fidelity(real[0], s[0][off:off + cnt], E2E_K, conditions=(real[2], s[2][off:off + cnt]), names=["met"])
        q.put((rank, res))
    except Exception as e:
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_subtype_fidelity_equals_single_process():
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
    ref = _device("inverted")[0]
    for _, r in res:
        assert list(r) == list(ref)
        for key, v in ref.items():
            if key in EXACT_KEYS or "_share_" in key:          # counts and shares: exact
                assert r[key] == v or (np.isnan(v) and np.isnan(r[key])), (key, r[key], v)
            elif np.isnan(v):
                assert np.isnan(r[key]), key
            else:                                              # double sums added in a different grouping
                assert abs(r[key] - v) <= 1e-12 * abs(v), (key, r[key], v)
    assert res[0][1] == res[1][1] or all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(res[0][1].values(), res[1][1].values()))


# ---- 6. validate_all --------------------------------------------------------------------------------------------------------------
def test_validate_all_carries_the_subtype_keys():
    import pandas as pd
    real, samplers = _samplers()
    x, y = real[0], samplers["faithful"][0]

    def frames(a):
        mut = pd.DataFrame((a[:, :10] > 0.5).astype(np.float32), columns=[f"M{i}" for i in range(10)])
        expr = pd.DataFrame(a[:, 10:120], columns=[f"G{i}" for i in range(110)])
        pw = pd.DataFrame(a[:, 120:], columns=[f"PW{i}" for i in range(10)])
        return mut, expr, pw

    val = BiologicalValidator(CONF)
    np.random.seed(5)
    plain = val.validate_all(*frames(x), *frames(y))
    np.random.seed(5)
    full = val.validate_all(*frames(x), *frames(y), subtypes=4)
    assert not any(k.startswith("subtype_") for k in plain)
    extra = [k for k in full if k not in plain]
    assert all(k.startswith("subtype_") for k in extra) and [k for k in full if k in plain] == list(plain)
    assert all(full[k] == pytest.approx(plain[k], rel=1e-9, abs=1e-12, nan_ok=True) for k in plain)      # double atomics: last-bit freedom
    both = np.concatenate([np.asarray(f.values, dtype=np.float32) for f in frames(x)], axis=1), np.concatenate(
        [np.asarray(f.values, dtype=np.float32) for f in frames(y)], axis=1)
    direct = val.subtype_fidelity(both[0], both[1], 4)
    assert extra == list(direct) and all(full[k] == direct[k] or (np.isnan(full[k]) and np.isnan(direct[k])) for k in extra)
    assert full["subtype_k"] == 4 and full["subtype_missing"] == 0
