"""GPU: the k-nearest-neighbour and ball-count kernels (osd_val_knn: EpiKnn on the fp32 Gram tiles + k_knn_refine + k_knn_sort;
osd_val_ball_counts: EpiBallCount) and precision / recall / density / coverage above them, against an fp64 brute force kept in this
file.

Both kernels judge the fp32 expanded form |r|^2 + |q|^2 - 2 r.q, whose error scales with the squared norms and not with the
distance: |expanded_fp32 - d2_64| <= C eps32 (|q|^2 + |r|^2) with tests/test_gpu_privacy.py's C = 13.72 (4 x the worst ratio numpy's own
fp32 expanded form shows on this data; its docstring has the figures).  So

  * slot s of a query's neighbour list is held to  d2_64(q, r_idx[s]) <= (s-th smallest fp64 d2) + margin  (of the s + 1 truly nearest
    rows, each is either in the list or was displaced by k rows that are at most two roundings farther), the returned distances --
    recomputed directly -- to the fp64 direct distance at rtol 1e-6;
  * a count is held between the fp64 counts with every pair's threshold lowered and raised by the pair's margin, and the test asserts
    that this band is narrow (<= 1 % of the counts), so that it cannot hide a failure;
  * on a grid of small integers every fp32 operation is exact, and everything -- indices, distances, counts, metrics, the `<=` at a
    radius and the smaller index at a tie -- is compared for equality."""
import ctypes as C_
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels, prdc_summary
from helpers import load_golden

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
C_BOUND = 4 * 3.43                 # tests/test_gpu_privacy.py's bound on the expanded form's error, in eps32 (|q|^2 + |r|^2)
KNN_CASES = [(5, 3, 8, 5),         # fewer candidates than k: padding
             (257, 300, 70, 5),    # ragged tiles on both sides, D % 4 != 0, a K tail
             (1100, 384, 64, 5),   # nine query tiles: the 8-way XCD tile order wraps; the aligned fast path
             (130, 700, 516, 1),   # six reference tiles: the seeding launch and the main launch; k = 1 against osd_val_nearest
             (130, 700, 516, 16)]  # the longest list
SHAPES = sorted({c[:3] for c in KNN_CASES})
CONF = {"evaluation": {}}
PRDC_KEYS = ["prdc_precision", "prdc_recall", "prdc_density", "prdc_coverage", "prdc_k"]


def _rows(rs, n, D):
    x = rs.standard_normal((n, D)).astype(np.float32)
    x[:, :D // 4] = (rs.random((n, D // 4)) < 0.3).astype(np.float32)      # a 0/1 mutation block in front of the normals
    return x


def _d2_matrix(q, r):
    a, b = q.astype(np.float64), r.astype(np.float64)
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)


def _margin(q, r):
    """C eps32 (|q|^2 + |r|^2) for every pair."""
    a, b = q.astype(np.float64), r.astype(np.float64)
    return C_BOUND * EPS32 * ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])


@functools.lru_cache(maxsize=None)
def _case(nq, nr, D):
    """(Q, R) float32 and the fp64 distance matrix [nq][nr] (expanded form in fp64: 1e-13 absolute at these norms)."""
    rs = np.random.default_rng(1000 * nq + nr + D)
    q, r = _rows(rs, nq, D), _rows(rs, nr, D)
    return q, r, _d2_matrix(q, r)


@functools.lru_cache(maxsize=None)
def _self_d2(nq, nr, D, which):
    """fp64 distances inside one cohort of _case, the diagonal at +inf."""
    x = _case(nq, nr, D)[which]
    d = _d2_matrix(x, x)
    d[np.arange(len(x)), np.arange(len(x))] = np.inf
    return d


def _kth_r2(d_self, k):
    """fp64 squared k-th-neighbour radius of every row (k cut to the rows there are)."""
    k = min(k, d_self.shape[1] - 1)
    return np.sort(d_self, axis=1)[:, k - 1]


def _kernels():
    return DeviceKernels(torch.device("cuda:0"))


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _knn(q, r, k, exclude=None):
    ex = None if exclude is None else _t(np.asarray(exclude), torch.int32)
    d2, idx = _kernels().knn(_t(q), _t(r), k, ex)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.is_cuda and idx.is_cuda
    assert tuple(d2.shape) == (q.shape[0], k) and tuple(idx.shape) == (q.shape[0], k)
    return d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _counts(q, r, r2_ref=None, r2_query=None):
    a, b = _kernels().ball_counts(_t(q), _t(r), None if r2_ref is None else _t(r2_ref, torch.float32),
                                  None if r2_query is None else _t(r2_query, torch.float32))
    for t, rad in ((a, r2_ref), (b, r2_query)):
        assert (t is None) == (rad is None)
        assert t is None or (t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == (q.shape[0],))
    return (None if a is None else a.cpu().numpy().astype(np.int64)), (None if b is None else b.cpu().numpy().astype(np.int64))


def _metrics(D, r2x, r2y, k, shift_x=0.0, shift_y=0.0):
    """fp64 precision / recall / density / coverage from D[i][j] = d2(x_i, y_j) and the squared radii, the thresholds moved by the
    [N][M] arrays (or scalars) shift_x (real balls) and shift_y (synthetic balls)."""
    in_x = D <= r2x[:, None] + shift_x                                     # y_j inside x_i's ball
    in_y = D <= r2y[None, :] + shift_y                                     # x_i inside y_j's ball
    rows = {"synth_in_real_balls": in_x.sum(0), "real_in_synth_balls": in_y.sum(1), "real_ball_synth": in_x.sum(1)}
    return prdc_summary(rows, k), rows


# ---- 1. integers: everything exact ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid():
    rs = np.random.default_rng(257300070)
    y = rs.integers(-2, 3, (257, 70)).astype(np.float32)      # synthetic
    x = rs.integers(-2, 3, (300, 70)).astype(np.float32)      # real
    y[:20] = x[:20]
    return x, y


def _expanded32(q, r):
    sq, sr = (q * q).sum(1, dtype=np.float32), (r * r).sum(1, dtype=np.float32)
    return np.maximum(sr[None, :] + sq[:, None] - np.float32(2) * (q @ r.T), np.float32(0))


def _lex_knn(D2, k):
    idx = np.argsort(D2, axis=1, kind="stable")[:, :k]       # ties to the smaller index
    return np.take_along_axis(D2, idx, 1), idx


def test_exact_on_an_integer_grid():
    x, y = _grid()
    k = 5
    Dyx, Dxx, Dyy = _d2_matrix(y, x), _d2_matrix(x, x), _d2_matrix(y, y)
    # the premise: on this data the fp32 expanded form IS the fp64 matrix
    for a, b, D in ((y, x, Dyx), (x, x, Dxx), (y, y, Dyy)):
        e = _expanded32(a, b)
        assert e.dtype == np.float32 and np.array_equal(e.astype(np.float64), D) and D.max() < 2 ** 24
    for D in (Dxx, Dyy):
        D[np.arange(len(D)), np.arange(len(D))] = np.inf
    d2, idx = _knn(y, x, k)
    rd, ri = _lex_knn(Dyx, k)
    assert np.array_equal(idx, ri) and np.array_equal(d2.astype(np.float64), rd)
    assert (idx[:20, 0] == np.arange(20)).all() and (d2[:20, 0] == 0).all()
    radii = []
    for a, D in ((x, Dxx), (y, Dyy)):                        # one operand, the diagonal excluded: the shared-norm path
        d2s, idxs = _knn(a, a, k, np.arange(len(a)))
        rd, ri = _lex_knn(D, k)
        assert np.array_equal(idxs, ri) and np.array_equal(d2s.astype(np.float64), rd)
        ties = int((rd[:, 1:] == rd[:, :-1]).sum())
        assert ties > 0                                      # the tie rule was exercised
        radii.append(d2s[:, k - 1].copy())
    r2x, r2y = radii
    # pairs exactly ON a radius: `<=` against `<` makes a difference
    on = int((Dyx == r2x[None, :].astype(np.float64)).sum() + (Dyx == r2y[:, None].astype(np.float64)).sum())
    print(f"grid: {on} pairs exactly on a radius, largest d2 {Dyx.max():.0f}")
    assert on > 20
    cr, cq = _counts(y, x, r2x, r2y)
    assert np.array_equal(cr, (Dyx <= r2x[None, :]).sum(1)) and np.array_equal(cq, (Dyx <= r2y[:, None]).sum(1))
    assert not np.array_equal(cr, (Dyx < r2x[None, :]).sum(1))
    only_r, none_q = _counts(y, x, r2_ref=r2x)
    none_r, only_q = _counts(y, x, r2_query=r2y)
    assert none_q is None and none_r is None and np.array_equal(only_r, cr) and np.array_equal(only_q, cq)
    ref, ref_rows = _metrics(Dyx.T, r2x.astype(np.float64), r2y.astype(np.float64), k)
    val = BiologicalValidator(CONF)
    got, rows = val.fidelity_diversity(x, y, k=k, return_rows=True)
    assert list(got) == PRDC_KEYS and got == ref
    for key in ref_rows:
        assert rows[key].dtype == np.int64 and np.array_equal(rows[key], ref_rows[key]), key
    assert np.array_equal(rows["real_radius"], np.sqrt(r2x.astype(np.float64)))
    assert np.array_equal(rows["synth_radius"], np.sqrt(r2y.astype(np.float64)))
    assert 0 < got["prdc_precision"] <= 1 and got["prdc_coverage"] >= 20 / 300
    # a function of the inputs alone
    d2b, idxb = _knn(y, x, k)
    assert np.array_equal(idx, idxb) and np.array_equal(d2.view(np.uint32), d2b.view(np.uint32))
    crb, cqb = _counts(y, x, r2x, r2y)
    assert np.array_equal(cr, crb) and np.array_equal(cq, cqb)
    assert val.fidelity_diversity(pd.DataFrame(x), torch.from_numpy(y).cuda(), k=k) == got


# ---- 2. knn on real-valued rows -------------------------------------------------------------------------------------------------
def _check_knn(q, r, D2, k, d2, idx, what):
    """The criterion of the module docstring for every (query, slot); D2 carries +inf where a candidate is excluded."""
    nq, nr = D2.shape
    n_cand = np.isfinite(D2).sum(1)
    srt = np.sort(D2, axis=1)
    worst = 0.0
    for s in range(k):
        have = n_cand > s
        assert (idx[~have, s] == -1).all() and np.isposinf(d2[~have, s]).all(), f"{what}: padding of slot {s}"
        if not have.any():
            continue
        rows, j = np.nonzero(have)[0], idx[have, s]
        assert ((j >= 0) & (j < nr)).all(), what
        assert np.isfinite(D2[rows, j]).all(), f"{what}: an excluded row came back"
        direct = ((q[rows].astype(np.float64) - r[j].astype(np.float64)) ** 2).sum(1)
        norms = (q[rows].astype(np.float64) ** 2).sum(1) + (r[j].astype(np.float64) ** 2).sum(1)
        excess = (direct - srt[rows, s]) / (EPS32 * norms)
        worst = max(worst, float(excess.max(initial=0.0)))
        assert (excess <= C_BOUND).all(), f"{what}: slot {s}"
        np.testing.assert_allclose(d2[rows, s], direct, rtol=1e-6, atol=0, err_msg=f"{what}: slot {s}")
    for i in range(nq):
        v = idx[i][idx[i] >= 0]
        assert len(np.unique(v)) == len(v), f"{what}: row {i} lists a neighbour twice"
    assert (d2[:, :-1] <= d2[:, 1:]).all(), f"{what}: not ascending"
    kk = min(k, nr)
    differ = int((idx[:, :kk] != _lex_knn(D2, kk)[1]).sum())
    print(f"{what}: worst excess over the fp64 order statistics {worst:.3f} eps32 (|q|^2 + |r|^2), bound {C_BOUND}; "
          f"{differ} of {nq * kk} slots differ from the fp64 order")


@pytest.mark.parametrize("nq,nr,D,k", KNN_CASES)
def test_knn_vs_fp64_brute_force(nq, nr, D, k):
    q, r, D2 = _case(nq, nr, D)
    d2, idx = _knn(q, r, k)
    _check_knn(q, r, D2, k, d2, idx, f"knn {nq}x{nr}x{D} k={k}")
    if nr < k:
        assert (idx[:, nr:] == -1).all() and np.isposinf(d2[:, nr:]).all() and (idx[:, :nr] >= 0).all()
    if k == 1:
        n2, ni = _kernels().nearest(_t(q), _t(r))
        k2, ki = _kernels().knn(_t(q), _t(r), 1)
        assert torch.equal(k2[:, 0], n2) and torch.equal(ki[:, 0], ni)


@pytest.mark.parametrize("nq,nr,D,k", [(257, 300, 70, 5), (130, 700, 516, 5)])
def test_knn_self_with_exclusion(nq, nr, D, k):
    """One operand with the diagonal excluded (the shared row norms), as fidelity_diversity calls it; 700 rows: both launches."""
    _, r, _ = _case(nq, nr, D)
    masked = _self_d2(nq, nr, D, 1)
    d2, idx = _knn(r, r, k, np.arange(nr))
    assert (idx != np.arange(nr)[:, None]).all()
    _check_knn(r, r, masked, k, d2, idx, f"self {nr}x{nr}x{D} k={k}")
    # excluding a row's nearest neighbour instead: the row finds itself first, at 0.0
    d2e, idxe = _knn(r, r, k, idx[:, 0])
    assert (idxe[:, 0] == np.arange(nr)).all() and (d2e[:, 0] == 0.0).all() and (idxe != idx[:, :1]).all()


# ---- 3. ball counts on real-valued rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nr,D", SHAPES)
def test_ball_counts_within_the_rounding_band(nq, nr, D):
    q, r, D2 = _case(nq, nr, D)
    r2_ref = _kth_r2(_self_d2(nq, nr, D, 1), 5).astype(np.float32)        # test-supplied radii: fp64 5th neighbour, rounded
    r2_query = _kth_r2(_self_d2(nq, nr, D, 0), 5).astype(np.float32)
    m = _margin(q, r)
    cr, cq = _counts(q, r, r2_ref, r2_query)
    total_hi = total_gap = 0
    for got, thr, name in ((cr, r2_ref.astype(np.float64)[None, :], "in_ref"), (cq, r2_query.astype(np.float64)[:, None], "in_query")):
        lo, hi = (D2 <= thr - m).sum(1), (D2 <= thr + m).sum(1)
        print(f"ball_counts {nq}x{nr}x{D} {name}: {int(hi.sum())} pairs inside, {int((hi - lo).sum())} within the margin, "
              f"{int((got != (D2 <= thr).sum(1)).sum())} rows differ from the fp64 count")
        assert ((lo <= got) & (got <= hi)).all(), name
        total_hi += int(hi.sum())
        total_gap += int((hi - lo).sum())
    assert total_gap <= 0.01 * total_hi                                    # the band cannot hide a failure
    assert nq < 100 or total_hi > 1000                                     # ... nor is there nothing to count
    # radii that hold nothing, and one that holds everything
    for bad in (np.nan, -1.0, -np.inf):
        zr, zq = _counts(q, r, np.full(nr, bad, dtype=np.float32), np.full(nq, bad, dtype=np.float32))
        assert (zr == 0).all() and (zq == 0).all(), bad
    ar, aq = _counts(q, r, np.full(nr, np.inf, dtype=np.float32), np.full(nq, np.inf, dtype=np.float32))
    assert (ar == nr).all() and (aq == nr).all()
    mixed = r2_ref.copy()
    mixed[::2] = np.nan                                                    # per row: the odd reference rows keep their balls
    mr, _ = _counts(q, r, r2_ref=mixed)
    lo = (D2[:, 1::2] <= (r2_ref.astype(np.float64)[None, :] - m)[:, 1::2]).sum(1)
    hi = (D2[:, 1::2] <= (r2_ref.astype(np.float64)[None, :] + m)[:, 1::2]).sum(1)
    assert ((lo <= mr) & (mr <= hi)).all()


# ---- 4. precision / recall / density / coverage end to end ----------------------------------------------------------------------
@pytest.mark.parametrize("nq,nr,D,shift", [(257, 300, 70, 0.0), (257, 300, 70, 0.5), (130, 700, 516, 0.0), (130, 700, 516, 0.15)])
def test_fidelity_diversity_vs_fp64(nq, nr, D, shift):
    """Real cohort = the case's nq query rows, synthetic = its nr reference rows (+ shift).  Every metric must lie in the fp64 band
    with every threshold moved by the pair's margin plus rtol 1e-6 on the radius."""
    k = 5
    x, r, _ = _case(nq, nr, D)
    y = (r + np.float32(shift)).astype(np.float32)
    Dxy = _d2_matrix(x, y)
    self_x, self_y = _d2_matrix(x, x), _d2_matrix(y, y)
    for d in (self_x, self_y):
        d[np.arange(len(d)), np.arange(len(d))] = np.inf
    r2x, r2y = _kth_r2(self_x, k), _kth_r2(self_y, k)
    m = _margin(x, y)
    ref, _ = _metrics(Dxy, r2x, r2y, k)
    lo, _ = _metrics(Dxy, r2x, r2y, k, -(m + 1e-6 * r2x[:, None]), -(m + 1e-6 * r2y[None, :]))
    hi, _ = _metrics(Dxy, r2x, r2y, k, m + 1e-6 * r2x[:, None], m + 1e-6 * r2y[None, :])
    got, rows = BiologicalValidator(CONF).fidelity_diversity(x, y, k=k, return_rows=True)
    print(f"prdc {nq}x{nr}x{D} shift {shift}: fp64 {ref}\n  got {got}\n  band {lo} .. {hi}")
    assert list(got) == PRDC_KEYS and got["prdc_k"] == k
    # the radii: the largest recomputed distance (rtol 1e-6) of a k-set that can differ from the true one by rows two roundings apart
    for name, a, r2 in (("real_radius", x, r2x), ("synth_radius", y, r2y)):
        sq = (a.astype(np.float64) ** 2).sum(1)
        got_r2 = rows[name] ** 2
        assert (got_r2 >= r2 * (1 - 1e-6)).all() and (got_r2 <= (r2 + 2 * C_BOUND * EPS32 * (sq + sq.max())) * (1 + 1e-6)).all(), name
    if (nq, nr, D) == (257, 300, 70):                                      # the fp64 figures this case was chosen by
        table = {0.0: (0.747, 0.790, 0.761, 0.969), 0.5: (0.223, 0.319, 0.085, 0.300)}[shift]
        assert [ref[key] for key in PRDC_KEYS[:4]] == pytest.approx(list(table), abs=6e-4)
    for key in PRDC_KEYS[:4]:
        assert hi[key] - lo[key] <= 2.0 / min(nq, nr), key                 # the band cannot hide a failure
        assert lo[key] <= got[key] <= hi[key], key
    if (nq, nr, D, shift) == (257, 300, 70, 0.5):                          # well away from 0 and 1: a swapped cohort or radius shows
        assert all(0.05 < ref[key] < 0.95 for key in PRDC_KEYS[:4]), ref
        assert abs(ref["prdc_recall"] - ref["prdc_precision"]) > 4.0 / min(nq, nr)
        swapped = BiologicalValidator(CONF).fidelity_diversity(y, x, k=k)      # the cohorts the other way round: recall's definition
        assert lo["prdc_recall"] <= swapped["prdc_precision"] <= hi["prdc_recall"]


REF_EVAL = {"evaluation": {"driver_genes": ["TP53", "RB1", "ATRX", "DLG2", "PTEN"], "mutually_exclusive_pairs": [["TP53", "MDM2"]],
                           "required_correlations": [{"mutation": "TP53", "pathway": "HALLMARK_P53_PATHWAY", "direction": "negative"},
                                                     {"mutation": "MYC", "pathway": "HALLMARK_MYC_TARGETS_V1", "direction": "positive"}]}}
CO_NAMES = ["TP53", "RB1", "ATRX", "PTEN", "MDM2", "MYC"] + [f"M{i}" for i in range(54)]
# validate_all's keys, in its order, before this feature
BASE_KEYS = ["mutation_frequency_correlation", "driver_gene_frequency_diff", "mutual_exclusivity_violation_rate",
             "cooccurrence_pattern_correlation", "real_pathway_coherence", "synthetic_pathway_coherence", "pathway_coherence_correlation",
             "mutation_expression_violation_rate", "ks_test_mean_pvalue", "ks_test_fraction_significant", "mmd",
             "wasserstein_distance_mean", "overall_biological_score"]


def test_validate_all_with_and_without_prdc(golden_dir):
    g = load_golden(golden_dir, "g9_validation")
    val = BiologicalValidator(REF_EVAL)
    genes = [f"G{i}" for i in range(40)]
    pw_cols = ["HALLMARK_P53_PATHWAY", "HALLMARK_MYC_TARGETS_V1"]
    pgm = pd.DataFrame(g["coh_member"], index=[f"G{i}" for i in range(45)], columns=[f"P{i}" for i in range(12)])
    frames = (pd.DataFrame(g["co_real"], columns=CO_NAMES), pd.DataFrame(g["coh_real"], columns=genes),
              pd.DataFrame(g["all_real_pw"], columns=pw_cols), pd.DataFrame(g["co_synth"], columns=CO_NAMES),
              pd.DataFrame(g["coh_synth"], columns=genes), pd.DataFrame(g["me_pw"], columns=pw_cols), pgm)
    np.random.seed(123)
    base = val.validate_all(*frames)
    assert list(base) == BASE_KEYS
    np.random.seed(123)
    full = val.validate_all(*frames, prdc=True, prdc_k=3)
    assert [k for k in full if not k.startswith("prdc_")] == BASE_KEYS
    assert [k for k in full if k.startswith("prdc_")] == PRDC_KEYS and len(full) == len(base) + 5
    for k in base:                                           # the MMD's double atomics commit in any order: last-bit freedom
        assert full[k] == pytest.approx(base[k], rel=1e-9, abs=1e-12), k
    real = np.concatenate([f.values for f in frames[:3]], axis=1)
    synth = np.concatenate([f.values for f in frames[3:6]], axis=1)
    alone = val.fidelity_diversity(real, synth, k=3)
    assert alone == {k: full[k] for k in PRDC_KEYS} and alone["prdc_k"] == 3
    assert all(0.0 <= alone[k] <= 1.0 for k in ("prdc_precision", "prdc_recall", "prdc_coverage")) and alone["prdc_density"] >= 0.0


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------
def test_boundary_arguments():
    lib = L.lib()
    q = torch.randn(6, 8, device="cuda")
    r = torch.randn(4, 8, device="cuda")
    d2 = torch.empty((6, 16), dtype=torch.float32, device="cuda")
    idx = torch.empty((6, 16), dtype=torch.int32, device="cuda")
    rad_r, rad_q = torch.ones(4, device="cuda"), torch.ones(6, device="cuda")
    out_r, out_q = torch.empty(6, dtype=torch.int32, device="cuda"), torch.empty(6, dtype=torch.int32, device="cuda")
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def knn(qp, nq, rp, nr, D, k, d2p, ip):
        return lib.osd_val_knn(stream, 0, qp, nq, rp, nr, D, k, None, d2p, ip)

    for k in (1, 5, 16):
        assert knn(L.ptr(q), 6, L.ptr(r), 4, 8, k, L.ptr(d2), L.ptr(idx)) == L.OSD_OK
    for k in (0, 17, -1):
        assert knn(L.ptr(q), 6, L.ptr(r), 4, 8, k, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert b"k must lie in [1, 16]" in lib.osd_last_error()
    assert knn(None, 6, L.ptr(r), 4, 8, 5, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert knn(L.ptr(q), 6, None, 4, 8, 5, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert knn(L.ptr(q), 6, L.ptr(r), 4, 8, 5, None, L.ptr(idx)) == L.OSD_EINVAL
    assert knn(L.ptr(q), 6, L.ptr(r), 4, 8, 5, L.ptr(d2), None) == L.OSD_EINVAL
    assert knn(L.ptr(q), 0, L.ptr(r), 4, 8, 5, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert knn(L.ptr(q), 6, L.ptr(r), 0, 8, 5, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert knn(L.ptr(q), 6, L.ptr(r), 4, 0, 5, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL

    def balls(qp, rp, rr, rq, orr, oq, nq=6, nr=4, D=8):
        return lib.osd_val_ball_counts(stream, 0, qp, nq, rp, nr, D, rr, rq, orr, oq)

    assert balls(L.ptr(q), L.ptr(r), L.ptr(rad_r), L.ptr(rad_q), L.ptr(out_r), L.ptr(out_q)) == L.OSD_OK
    assert balls(L.ptr(q), L.ptr(r), L.ptr(rad_r), None, L.ptr(out_r), None) == L.OSD_OK
    assert balls(L.ptr(q), L.ptr(r), None, L.ptr(rad_q), None, L.ptr(out_q)) == L.OSD_OK
    assert balls(L.ptr(q), L.ptr(r), None, None, None, None) == L.OSD_EINVAL                      # no radius
    assert balls(L.ptr(q), L.ptr(r), None, None, L.ptr(out_r), L.ptr(out_q)) == L.OSD_EINVAL
    assert balls(L.ptr(q), L.ptr(r), L.ptr(rad_r), None, None, None) == L.OSD_EINVAL              # a radius without its output
    assert balls(L.ptr(q), L.ptr(r), L.ptr(rad_r), L.ptr(rad_q), L.ptr(out_r), None) == L.OSD_EINVAL
    assert balls(None, L.ptr(r), L.ptr(rad_r), None, L.ptr(out_r), None) == L.OSD_EINVAL
    assert balls(L.ptr(q), None, L.ptr(rad_r), None, L.ptr(out_r), None) == L.OSD_EINVAL
    assert balls(L.ptr(q), L.ptr(r), L.ptr(rad_r), None, L.ptr(out_r), None, nq=0) == L.OSD_EINVAL
    assert balls(L.ptr(q), L.ptr(r), L.ptr(rad_r), None, L.ptr(out_r), None, D=0) == L.OSD_EINVAL
    k = _kernels()
    with pytest.raises(ValueError):
        k.knn(q, r, 0)
    with pytest.raises(ValueError):
        k.knn(q, r, 17)
    with pytest.raises(ValueError):
        k.knn(q, torch.zeros(4, 7, device="cuda"), 2)
    with pytest.raises(ValueError):
        k.ball_counts(q, r)
    with pytest.raises(ValueError):
        k.ball_counts(q, r, r2_ref=rad_q)                                  # one radius per reference row
    val = BiologicalValidator(CONF)
    bad = np.ones((9, 8), dtype=np.float32)
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        val.fidelity_diversity(bad, np.ones((9, 8), dtype=np.float32), k=3)
    bad[2, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        val.fidelity_diversity(np.ones((9, 8), dtype=np.float32), bad, k=3)
