"""GPU: the privacy audit's nearest-record kernel (osd_val_nearest: EpiNearest on the fp32 Gram tiles + k_nearest_refine) and
the Python layers above it, against an fp64 brute force kept in this file.

The kernel ranks the candidates by the fp32 expanded form |r|^2 + |q|^2 - 2 r.q, whose error scales with the squared norms and
not with the distance.  So the returned index j is held to "a nearest neighbour up to that rounding":

    d2_64(q, r_j) <= min_j' d2_64(q, r_j') + C * eps32 * (|q|^2 + |r_j|^2),       eps32 = 2^-23

and the returned distance, which is recomputed directly, to d2_64(q, r_j) at rtol 1e-6.  C: numpy's own fp32 expanded form
(fp32 row norms, fp32 matmul) on the data of ``_case`` shows a worst |expanded_fp32 - d2_64| / (eps32 (|q|^2 + |r|^2)) of 3.43
(0.78, 2.34, 2.05 and 1.42 in the order of SHAPES; 3.43 and 3.16 on the two cases with planted copies); 4 x that for the different
summation order of the MFMA K loop gives C = 13.72.  On the CPU the fp32 expanded form picks the fp64 argmin in every row of
these cases: the bound is there for the summation order only."""
import ctypes as C_
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels
from helpers import load_golden

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
C_BOUND = 4 * 3.43                 # 4 x the worst ratio of numpy's fp32 expanded form, see the module docstring
SHAPES = [(5, 3, 8),               # less than one tile
          (257, 300, 70),          # ragged tiles on both sides, D % 4 != 0, a K tail
          (1100, 384, 64),         # nine query tiles: the 8-way XCD tile order wraps; the aligned fast path
          (130, 700, 516)]         # six reference tiles, D % 32 != 0


def _rows(rs, n, D):
    x = rs.standard_normal((n, D)).astype(np.float32)
    x[:, :D // 4] = (rs.random((n, D // 4)) < 0.3).astype(np.float32)      # a 0/1 mutation block in front of the normals
    return x


@functools.lru_cache(maxsize=None)
def _case(nq, nr, D, planted=False):
    """(Q, R) float32 and the fp64 distance matrix [nq][nr] (expanded form in fp64: 1e-13 absolute at these norms)."""
    rs = np.random.default_rng(1000 * nq + nr + D)
    q, r = _rows(rs, nq, D), _rows(rs, nr, D)
    if planted:
        q[:5] = r[10:15]
        q[5:10] = r[20:25] + np.float32(1e-3) * rs.standard_normal((5, D)).astype(np.float32)
    return q, r, _d2_matrix(q, r)


def _d2_matrix(q, r):
    a, b = q.astype(np.float64), r.astype(np.float64)
    return np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)


def _d2_direct(q, r, j):
    return ((q.astype(np.float64) - r.astype(np.float64)[j]) ** 2).sum(1)


def _kernels():
    return DeviceKernels(torch.device("cuda:0"))


def _nearest(q, r, exclude=None):
    ex = None if exclude is None else torch.as_tensor(np.asarray(exclude), dtype=torch.int32).cuda()
    d2, idx = _kernels().nearest(torch.from_numpy(q).cuda(), torch.from_numpy(r).cuda(), ex)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.is_cuda and idx.is_cuda
    return d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _check(q, r, D2, d2, idx, what):
    """The criterion of the module docstring, for every query; D2 carries +inf where a candidate is excluded."""
    assert ((idx >= 0) & (idx < r.shape[0])).all(), what
    direct = _d2_direct(q, r, idx)
    assert np.isfinite(D2[np.arange(len(idx)), idx]).all(), f"{what}: an excluded row came back"
    norms = (q.astype(np.float64) ** 2).sum(1) + (r.astype(np.float64)[idx] ** 2).sum(1)
    excess = (direct - D2.min(1)) / (EPS32 * norms)
    print(f"{what}: worst excess over the fp64 minimum {excess.max():.3f} eps32 (|q|^2 + |r|^2), bound {C_BOUND}; "
          f"{int((idx != D2.argmin(1)).sum())} of {len(idx)} indices differ from the fp64 argmin")
    assert (excess <= C_BOUND).all(), what
    np.testing.assert_allclose(d2, direct, rtol=1e-6, atol=0, err_msg=what)


@pytest.mark.parametrize("nq,nr,D", SHAPES)
def test_nearest_vs_fp64_brute_force(nq, nr, D):
    q, r, D2 = _case(nq, nr, D)
    d2, idx = _nearest(q, r)
    _check(q, r, D2, d2, idx, f"nearest {nq}x{nr}x{D}")


@pytest.mark.parametrize("nq,nr,D", [(257, 300, 70), (130, 700, 516)])
def test_copies_and_near_copies(nq, nr, D):
    """Exact copies come back as exactly 0.0; near copies (true d2 ~ 1e-6 D, below the expanded form's error) at rtol 1e-6."""
    q, r, D2 = _case(nq, nr, D, True)
    d2, idx = _nearest(q, r)
    assert idx[:5].tolist() == list(range(10, 15)) and (d2[:5] == 0.0).all()
    assert idx[5:10].tolist() == list(range(20, 25))
    near = _d2_direct(q[5:10], r, np.arange(20, 25))
    assert (near > 0).all() and (near < 2e-6 * D).all()
    np.testing.assert_allclose(d2[5:10], near, rtol=1e-6, atol=0)
    _check(q, r, D2, d2, idx, f"planted {nq}x{nr}x{D}")


def test_exclusion():
    _, r, _ = _case(257, 300, 70)
    n = r.shape[0]
    D2 = _d2_matrix(r, r)
    masked = D2.copy()
    masked[np.arange(n), np.arange(n)] = np.inf
    d2, idx = _nearest(r, r, np.arange(n))
    assert (idx != np.arange(n)).all()
    _check(r, r, masked, d2, idx, "self, diagonal excluded")
    # excluding the first answer instead of the diagonal: every row finds itself
    d2s, idxs = _nearest(r, r, idx)
    assert (idxs == np.arange(n)).all() and (d2s == 0.0).all()
    # two passes over distinct operands: the second one is the second order statistic
    q, r2, Dq = _case(257, 300, 70, True)
    d2a, ia = _nearest(q, r2)
    second = Dq.copy()
    second[np.arange(len(ia)), ia] = np.inf
    d2b, ib = _nearest(q, r2, ia)
    assert (ib != ia).all()
    _check(q, r2, second, d2b, ib, "second pass")
    assert (d2b[:5] > 0).all()                               # the planted copies' runner-up is a different patient
    # values outside [0, nr) exclude nothing
    for ex in (np.full(len(ia), -1), np.full(len(ia), r2.shape[0] + 5)):
        d2c, ic = _nearest(q, r2, ex)
        assert np.array_equal(ic, ia) and np.array_equal(d2c, d2a)
    # no candidate at all
    d2n, idn = _nearest(q[:7], r2[:1], np.zeros(7))
    assert (idn == -1).all() and np.isposinf(d2n).all()
    d2o, ido = _nearest(q[:7], r2[:1], np.array([0, 1, -1, 0, 5, 0, 0]))
    assert ido.tolist() == [-1, 0, 0, -1, 0, -1, -1] and np.isposinf(d2o[[0, 3, 5, 6]]).all() and np.isfinite(d2o[[1, 2, 4]]).all()


def test_ties_and_determinism():
    q, r, _ = _case(257, 300, 70)
    r = r.copy()
    r[200] = r[7]                                            # identical records in two different reference tiles
    query = np.ascontiguousarray(np.concatenate([r[7:8], q[:3]]))
    d2, idx = _nearest(query, r)
    assert idx[0] == 7 and d2[0] == 0.0
    d2, idx = _nearest(query, r, np.array([7, -1, -1, -1]))
    assert idx[0] == 200 and d2[0] == 0.0
    d2, idx = _nearest(query, r, np.array([200, -1, -1, -1]))
    assert idx[0] == 7 and d2[0] == 0.0
    q, r, _ = _case(1100, 384, 64)
    a, b = _nearest(q, r), _nearest(q, r)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# ---- privacy_audit against a numpy reference ------------------------------------------------------------------------
AUDIT_SEED = 1                     # passes both conditions asserted below on the fp64 reference (seeds 0 and 3 do not)


@functools.lru_cache(maxsize=None)
def _audit_data(seed=AUDIT_SEED, n_train=300, n_hold=150, n_synth=260, D=70):
    """Six Gaussian clusters with centres of scale 2; a fifth of the synthetic rows are train rows + 0.3 noise, the first four
    exact copies."""
    rs = np.random.default_rng(seed)
    centres = 2.0 * rs.standard_normal((6, D))

    def cohort(n):
        return (centres[rs.integers(0, 6, n)] + rs.standard_normal((n, D))).astype(np.float32)

    train, hold, synth = cohort(n_train), cohort(n_hold), cohort(n_synth)
    n_mem = n_synth // 5
    src = rs.permutation(n_train)[:n_mem]
    synth[:n_mem] = train[src] + np.float32(0.3) * rs.standard_normal((n_mem, D)).astype(np.float32)
    synth[:4] = train[src[:4]]
    return train, hold, synth


def _two_smallest(D2):
    part = np.partition(D2, 2, axis=1)[:, :3]
    part.sort(axis=1)
    return part                                              # the three smallest of every row, ascending


def _audit_reference(train, hold, synth):
    """fp64 rows and summary, and the two conditions under which an fp32 kernel must reproduce them exactly."""
    Dt, Dh, Dr = _d2_matrix(synth, train), _d2_matrix(synth, hold), _d2_matrix(train, train)
    Dr[np.arange(len(train)), np.arange(len(train))] = np.inf
    match = Dt.argmin(1)
    # exact d2 of the winners (the matrix is the expanded form in fp64: fine for ranking, not for a distance of 0)
    dcr = np.sqrt(_d2_direct(synth, train, match))
    masked = Dt.copy()
    masked[np.arange(len(synth)), match] = np.inf
    second = np.sqrt(_d2_direct(synth, train, masked.argmin(1)))
    real_nn = np.sqrt(_d2_direct(train, train, Dr.argmin(1)))
    dcr_h = np.sqrt(_d2_direct(synth, hold, Dh.argmin(1)))
    rows = {"dcr": dcr, "match": match, "second": second, "real_nn": real_nn, "dcr_holdout": dcr_h}

    def rel_margin(a, b):
        return float((np.abs(a - b) / np.maximum(np.maximum(a, b), 1e-300)).min())

    boundary = min(rel_margin(dcr, real_nn[match]), rel_margin(dcr, dcr_h))
    # uniqueness of every index the kernel has to pick -- nearest and second nearest train row, nearest holdout row, nearest other
    # train row -- by the margin of the module docstring: gap to the next candidate > C eps32 (|q|^2 + |r|^2), |r|^2 taken as the
    # largest norm of the cohort
    unique = np.inf
    for D2, qs, rsq, depth in ((Dt, synth, train, 2), (Dh, synth, hold, 1), (Dr, train, train, 1)):
        three = _two_smallest(D2)
        norms = (qs.astype(np.float64) ** 2).sum(1) + (rsq.astype(np.float64) ** 2).sum(1).max()
        for lvl in range(depth):
            unique = min(unique, float(((three[:, lvl + 1] - three[:, lvl]) / (C_BOUND * EPS32 * norms)).min()))
    nndr = np.divide(dcr, second, out=np.zeros_like(dcr), where=second > 0)
    summary = {
        "privacy_dcr_min": dcr.min(), "privacy_dcr_p05": np.quantile(dcr, 0.05), "privacy_dcr_median": np.median(dcr),
        "privacy_exact_copy_fraction": np.mean(dcr == 0),
        "privacy_nndr_p05": np.quantile(nndr, 0.05), "privacy_nndr_median": np.median(nndr),
        "privacy_real_nn_median": np.median(real_nn),
        "privacy_closer_than_real_nn_fraction": np.mean(dcr < real_nn[match]),
        "privacy_holdout_dcr_median": np.median(dcr_h),
        "privacy_closer_to_train_fraction": np.mean(np.where(dcr == dcr_h, 0.5, (dcr < dcr_h).astype(np.float64))),
    }
    return rows, {k: float(v) for k, v in summary.items()}, boundary, unique


PRIVACY_KEYS = ["privacy_dcr_min", "privacy_dcr_p05", "privacy_dcr_median", "privacy_exact_copy_fraction", "privacy_nndr_p05",
                "privacy_nndr_median", "privacy_real_nn_median", "privacy_closer_than_real_nn_fraction", "privacy_holdout_dcr_median",
                "privacy_closer_to_train_fraction"]
CONF = {"evaluation": {}}


def test_privacy_audit_vs_numpy_reference():
    train, hold, synth = _audit_data()
    ref_rows, ref, boundary, unique = _audit_reference(train, hold, synth)
    # the data must leave the fp32 kernel no decision to get wrong: no row near a boundary, every neighbour unique
    assert boundary > 1e-5, boundary
    assert unique > 1.0, unique
    # ... and the test must not be vacuous
    assert ref["privacy_exact_copy_fraction"] == 4 / 260
    assert 0.3 < ref["privacy_closer_than_real_nn_fraction"] < 0.5
    assert 0.65 < ref["privacy_closer_to_train_fraction"] < 0.85
    val = BiologicalValidator(CONF)
    got, rows = val.privacy_audit(train, synth, hold, return_rows=True)
    assert list(got) == PRIVACY_KEYS
    for k in ("privacy_exact_copy_fraction", "privacy_closer_than_real_nn_fraction", "privacy_closer_to_train_fraction"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in PRIVACY_KEYS:
        assert got[k] == pytest.approx(ref[k], rel=1e-5, abs=0), (k, got[k], ref[k])
    assert list(rows) == ["dcr", "match", "second", "real_nn", "dcr_holdout"]
    assert np.array_equal(rows["match"], ref_rows["match"])
    for k in ("dcr", "second", "real_nn", "dcr_holdout"):
        np.testing.assert_allclose(rows[k], ref_rows[k], rtol=1e-6, atol=0, err_msg=k)
    # frames and device tensors go through the same door; without a holdout the two holdout keys are absent
    again = val.privacy_audit(pd.DataFrame(train), torch.from_numpy(synth).cuda())
    assert list(again) == PRIVACY_KEYS[:8] and all(again[k] == got[k] for k in again)


REF_EVAL = {"evaluation": {"driver_genes": ["TP53", "RB1", "ATRX", "DLG2", "PTEN"], "mutually_exclusive_pairs": [["TP53", "MDM2"]],
                           "required_correlations": [{"mutation": "TP53", "pathway": "HALLMARK_P53_PATHWAY", "direction": "negative"},
                                                     {"mutation": "MYC", "pathway": "HALLMARK_MYC_TARGETS_V1", "direction": "positive"}]}}
CO_NAMES = ["TP53", "RB1", "ATRX", "PTEN", "MDM2", "MYC"] + [f"M{i}" for i in range(54)]
# validate_all's keys, in its order, before this feature
BASE_KEYS = ["mutation_frequency_correlation", "driver_gene_frequency_diff", "mutual_exclusivity_violation_rate",
             "cooccurrence_pattern_correlation", "real_pathway_coherence", "synthetic_pathway_coherence", "pathway_coherence_correlation",
             "mutation_expression_violation_rate", "ks_test_mean_pvalue", "ks_test_fraction_significant", "mmd",
             "wasserstein_distance_mean", "overall_biological_score"]


def test_validate_all_with_and_without_privacy(golden_dir):
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
    assert set(base) == {k[4:] for k in g if k.startswith("all.") and k != "all_real_pw"}
    # a holdout with the cohort's columns (only the keys are under test here: the back third of the real rows, noised)
    rs = np.random.default_rng(5)
    cut = (2 * len(frames[0])) // 3
    holdout = tuple(f.iloc[cut:].reset_index(drop=True) + 0.1 * rs.standard_normal(f.iloc[cut:].shape) for f in frames[:3])
    np.random.seed(123)
    full = val.validate_all(*frames, privacy=True, holdout=holdout)
    assert [k for k in full if not k.startswith("privacy_")] == BASE_KEYS
    assert [k for k in full if k.startswith("privacy_")] == PRIVACY_KEYS and len(full) == len(base) + 10
    for k in base:                                           # the MMD's double atomics commit in any order: last-bit freedom
        assert full[k] == pytest.approx(base[k], rel=1e-9, abs=1e-12), k
    assert all(np.isfinite(full[k]) for k in PRIVACY_KEYS)
    np.random.seed(123)
    eight = val.validate_all(*frames, privacy=True)
    assert [k for k in eight if k.startswith("privacy_")] == PRIVACY_KEYS[:8] and len(eight) == len(base) + 8


def test_boundary_arguments():
    lib = L.lib()
    q = torch.randn(6, 8, device="cuda")
    r = torch.randn(4, 8, device="cuda")
    d2 = torch.empty(6, dtype=torch.float32, device="cuda")
    idx = torch.empty(6, dtype=torch.int32, device="cuda")
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(qp, nq, rp, nr, D, d2p, ip):
        return lib.osd_val_nearest(stream, 0, qp, nq, rp, nr, D, None, d2p, ip)

    assert call(L.ptr(q), 6, L.ptr(r), 4, 8, L.ptr(d2), L.ptr(idx)) == L.OSD_OK
    assert call(None, 6, L.ptr(r), 4, 8, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert call(L.ptr(q), 6, None, 4, 8, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert call(L.ptr(q), 6, L.ptr(r), 4, 8, None, L.ptr(idx)) == L.OSD_EINVAL
    assert call(L.ptr(q), 6, L.ptr(r), 4, 8, L.ptr(d2), None) == L.OSD_EINVAL
    assert call(L.ptr(q), 0, L.ptr(r), 4, 8, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert call(L.ptr(q), 6, L.ptr(r), 0, 8, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert call(L.ptr(q), 6, L.ptr(r), 4, 0, L.ptr(d2), L.ptr(idx)) == L.OSD_EINVAL
    assert b"bad argument" in lib.osd_last_error()
    val = BiologicalValidator(CONF)
    train, synth = np.ones((5, 8), dtype=np.float32), np.zeros((4, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        val.privacy_audit(train, synth[:, :7])
    with pytest.raises(ValueError):
        val.privacy_audit(train, synth, np.ones((3, 9), dtype=np.float32))
    bad = synth.copy()
    bad[2, 3] = np.nan
    with pytest.raises(ValueError):
        val.privacy_audit(train, bad)
    bad[2, 3] = np.inf
    with pytest.raises(ValueError):
        val.privacy_audit(bad, synth)
    with pytest.raises(ValueError):
        _kernels().nearest(torch.zeros(3, 8, device="cuda"), torch.zeros(3, 7, device="cuda"))
