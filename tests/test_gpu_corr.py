"""GPU: the centred Gram kernel (osd_val_centered_gram: cov_gram_kernel + cov_gram_reduce, csrc/corr.hip), the correlation comparison
(osd_val_corr_compare) and ``BiologicalValidator.correlation_fidelity`` / ``validate_all(correlation=True)`` above them, against the
double-precision numpy restatement of tests/corr_helpers.py.

Shapes (rows, D): (33, 6), (257, 130), (1000, 258), (4099, 516) -- D < 128 and rows barely above one 32-row stage; one-row tails (33,
257); D % 4 == 2 (130, 258: the padded copy); 4099 rows at 15 tiles: eight row slices, seven of 544 rows -- three accumulator runs,
256 + 256 + 32 -- and a last one of 291 rows that ends in a 3-row tail.

  * integers 0..4 with integer centres: every difference, product and run sum is an integer below 2^24, so G must EQUAL the int64
    result -- a dropped or doubled row, an unmasked tail row, an unmirrored tile or a column read past D shows as a wrong integer;
  * real-valued cohorts: r_dev = G_ij / sqrt(G_ii G_jj) against r_64 computed in double from the same fp32 inputs.

    Measured max |r_dev - r_64|: 1.05e-7 (33 x 6), 5.10e-7 (257 x 130), 1.05e-6 (1000 x 258), 2.32e-6 (4099 x 516) -- it grows with
    the rows per accumulator run (32, 64, 128, 256), not with the rows; R_OBSERVED = 2.315e-6 is the largest.  Asserted: R_TOL =
    4 x that = 9.26e-6 -- other seeds, and the order freedom inside the MFMA.  It may not exceed R_CEILING = 2 (OSD_COV_SLAB_ROWS + 4) 2^-24,
    what the rounding model allows: one rounding per centred value, per product and per accumulate within a run (Cauchy-Schwarz
    bounds sum |c_i c_j| by sqrt(G_ii G_jj)), the same relative error on the two diagonal elements, double precision above the run."""
import ctypes as C_
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import (COV_SLAB_ROWS, BiologicalValidator, DeviceKernels, corr_summary, frechet_distance,
                                                        sharded_centered_gram)
from corr_helpers import FRECHET_KEYS, SUMMARY_KEYS, cohorts, compare_stats, corr_of_gram, gram64, pair_masks, summary_oracle
from helpers import load_golden

pytestmark = pytest.mark.gpu

SHAPES = [(33, 6), (257, 130), (1000, 258), (4099, 516)]
R_OBSERVED = 2.315e-6                                   # max |r_dev - r_64| measured over SHAPES
R_TOL = 4 * R_OBSERVED                                 # asserted
R_CEILING = 2 * (COV_SLAB_ROWS + 4) * 2.0 ** -24       # 3.1e-5 at 256 rows per run
CONF = {"evaluation": {}}
E2E_CASES = [(33, 40, 6), (257, 300, 130), (4099, 2051, 516)]


def _kernels():
    return DeviceKernels(torch.device("cuda:0"))


def _t(a):
    return torch.as_tensor(np.array(a)).cuda()                # a copy: the cached cohorts are read-only


# ---- 1. integers: exact ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_case(rows, D):
    rs = np.random.default_rng(97 * rows + D)
    x = rs.integers(0, 5, (rows, D)).astype(np.float32)
    c = np.where(np.arange(D) % 3 == 1, 2.0, 0.0).astype(np.float32)           # integer centres 0 and 2
    z = x.astype(np.int64) - c.astype(np.int64)
    return x, c, z.T @ z


@pytest.mark.parametrize("layout", ["dense", "slice_unaligned", "slice_aligned"])
@pytest.mark.parametrize("rows,D", SHAPES)
def test_exact_on_integers(rows, D, layout):
    x, c, ref = _int_case(rows, D)
    assert np.abs(ref).max() < 2 ** 24 and 16 * COV_SLAB_ROWS < 2 ** 24
    if layout == "dense":
        t = _t(x)
    else:                                       # a column slice of a wider matrix full of 1000s: ld > D, neighbours must not leak in
        off = 1 if layout == "slice_unaligned" else 4
        width = (off + D + 8) // 4 * 4 + (1 if layout == "slice_unaligned" else 0)
        big = torch.full((rows, width), 1000.0, device="cuda")
        big[:, off:off + D] = _t(x)
        t = big[:, off:off + D]
        assert t.stride(0) == width > D and (t.data_ptr() % 16 == 0) == (layout == "slice_aligned")
    G = _kernels().centered_gram(t, c)
    assert G.dtype == torch.float64 and G.is_cuda and tuple(G.shape) == (D, D)
    g = G.cpu().numpy()
    assert np.array_equal(g, g.T)
    assert np.array_equal(g, ref.astype(np.float64)), f"{int((g != ref).sum())} of {D * D} entries differ"


# ---- 2. same bits twice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", SHAPES[2:])
def test_same_bits_twice(rows, D):
    x, _ = cohorts(rows, rows, D)
    t = _t(x)
    c = x.astype(np.float64).mean(0)
    a, b = _kernels().centered_gram(t, c), _kernels().centered_gram(t, c)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a, a.T)
    st = [_kernels().corr_compare(a, b, [0, D], 0.3) for _ in range(2)]
    assert st[0]["sum_abs"][0] == 0.0 and st[0]["max_abs"][0] == 0.0 and st[0]["pairs"][0] == D * (D - 1) // 2
    assert all(np.array_equal(st[0][k], st[1][k]) for k in st[0])


# ---- 3. against double precision ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _r_error(rows, D):
    """max |r_dev - r_64| of both cohorts of the shape, and the relative error of the Gram diagonal."""
    worst = worst_diag = 0.0
    for x in cohorts(rows, rows, D):
        _, G64 = gram64(x)
        n, mu, G = sharded_centered_gram(ShardComm(False), _kernels(), _t(x))
        g = G.cpu().numpy()
        assert n == rows and np.array_equal(g, g.T)
        r64, live = corr_of_gram(G64)
        rdev, live_dev = corr_of_gram(g)
        assert live.all() and live_dev.all()
        worst = max(worst, float(np.abs(rdev - r64).max()))
        worst_diag = max(worst_diag, float(np.abs(np.diag(g) / np.diag(G64) - 1.0).max()))
    return worst, worst_diag


def test_tolerance_is_inside_the_rounding_model():
    assert R_TOL == 4 * R_OBSERVED and R_TOL <= R_CEILING


@pytest.mark.parametrize("rows,D", SHAPES)
def test_correlations_vs_double(rows, D):
    err, err_diag = _r_error(rows, D)
    print(f"centered_gram {rows}x{D}: max |r_dev - r_64| = {err:.3e}, max relative error of G_ii = {err_diag:.3e}; "
          f"asserted {R_TOL:.3e}, ceiling {R_CEILING:.3e}")
    assert err <= R_TOL and err_diag <= R_CEILING


# ---- 4. corr_compare against numpy on the device's own Gram matrices ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_grams(n_real, n_synth, D, constant=True):
    x, y = (a.copy() for a in cohorts(n_real, n_synth, D))
    if constant and D > 8:
        x[:, 3] = 1.5                                                          # a constant column in the real cohort
    out = []
    for a in (x, y):
        n, mu, G = sharded_centered_gram(ShardComm(False), _kernels(), _t(a))
        out.append((n, mu, G))
    return x, y, out


def _bounds(D):
    return {6: [0, 2, 5, 6], 130: [0, 37, 101, 130], 516: [0, 45, 300, 516]}[D]


@pytest.mark.parametrize("n_real,n_synth,D", E2E_CASES[1:])
def test_corr_compare_vs_numpy(n_real, n_synth, D):
    _, _, ((_, _, Gr), (_, _, Gs)) = _device_grams(n_real, n_synth, D)
    gr, gs = Gr.cpu().numpy(), Gs.cpu().numpy()
    bounds, strong = _bounds(D), 0.3
    assert any(b % 32 for b in bounds[1:-1])
    # the premise of exact counts: no pair sits on the strong threshold or on r_synth = 0
    rr, live_r = corr_of_gram(gr)
    rs, live_s = corr_of_gram(gs)
    live = live_r & live_s
    assert (~live).sum() == 1 and not live[3] and gr[3, 3] <= 0.0
    m = np.triu(np.ones((D, D), dtype=bool), 1) & live[:, None] & live[None, :]
    assert np.abs(np.abs(rr[m]) - strong).min() > 1e-9 and np.abs(rs[m]).min() > 1e-9
    ref = compare_stats(gr, gs, bounds, strong)
    got = _kernels().corr_compare(Gr, Gs, bounds, strong)
    assert set(got) == set(ref) and got["constant_columns"] == ref["constant_columns"] == 1
    assert int(ref["pairs"].sum()) == (D - 1) * (D - 2) // 2 and (ref["pairs"] > 0).all() and ref["strong_pairs"].sum() > 50
    for k in ("pairs", "strong_pairs", "strong_agree"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["max_abs"], ref["max_abs"])
    for k in ("sum_abs", "sum_sq", "strong_sum_abs"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=0, err_msg=k)
    one = _kernels().corr_compare(Gr, Gs, [0, D], strong)                      # one block = the sum of the six
    assert one["pairs"][0] == ref["pairs"].sum() and one["strong_agree"][0] == ref["strong_agree"].sum()
    assert one["max_abs"][0] == ref["max_abs"].max()
    np.testing.assert_allclose(one["sum_sq"][0], ref["sum_sq"].sum(), rtol=1e-12)
    none = _kernels().corr_compare(Gr, Gs, bounds, 2.0)                        # nothing is that strong
    assert none["strong_pairs"].sum() == 0 and none["strong_sum_abs"].sum() == 0.0 and np.array_equal(none["pairs"], ref["pairs"])


# ---- 5. correlation_fidelity end to end -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_real,n_synth,D", E2E_CASES)
def test_correlation_fidelity_vs_double(n_real, n_synth, D):
    x, y = cohorts(n_real, n_synth, D)
    bounds, names, strong = _bounds(D), ["mutations", "expression", "pathways"], 0.3
    blocks = {nm: bounds[i + 1] - bounds[i] for i, nm in enumerate(names)}
    (mu_x, Gx), (mu_y, Gy) = gram64(x), gram64(y)
    rr, live_r = corr_of_gram(Gx)
    rs, live_s = corr_of_gram(Gy)
    assert live_r.all() and live_s.all()
    # pairs whose strong / sign verdict the device's rounding may turn: left out of the counts on both sides
    skip = (np.abs(np.abs(rr) - strong) <= R_TOL) | (np.abs(rs) <= R_TOL)
    iu = np.triu(np.ones((D, D), dtype=bool), 1)
    left_out = int((skip & iu).sum())
    ref_stats = compare_stats(Gx, Gy, bounds, strong, skip=skip)
    ref = summary_oracle(compare_stats(Gx, Gy, bounds, strong), names)
    val = BiologicalValidator(CONF)
    got, mats = val.correlation_fidelity(x, y, blocks=blocks, strong=strong, frechet=True, return_matrices=True)
    assert list(got) == list(ref) + FRECHET_KEYS and len(got) == len(SUMMARY_KEYS) + 6 + 3
    pairs = D * (D - 1) // 2
    print(f"correlation_fidelity {n_real}+{n_synth}x{D}: {left_out} of {pairs} pairs left out of the counts; fp64 {ref}\n  got {got}")
    assert left_out <= 0.01 * pairs and (D > 6 or left_out == 0)
    assert got["corr_pairs"] == pairs and got["corr_constant_columns"] == 0 and mats["real_rows"] == n_real and mats["synth_rows"] == n_synth
    # counts: the device's verdicts, recomputed from its own matrices (test 4 ties the kernel to them), without the pairs in the band
    dev_stats = compare_stats(mats["real_gram"].cpu().numpy(), mats["synth_gram"].cpu().numpy(), bounds, strong, skip=skip)
    assert np.array_equal(dev_stats["strong_pairs"], ref_stats["strong_pairs"])
    assert np.array_equal(dev_stats["strong_agree"], ref_stats["strong_agree"])
    assert abs(got["corr_strong_pairs"] - int(ref_stats["strong_pairs"].sum())) <= left_out
    assert np.array_equal(mats["stats"]["strong_pairs"], compare_stats(mats["real_gram"].cpu().numpy(), mats["synth_gram"].cpu().numpy(),
                                                                       bounds, strong)["strong_pairs"])
    # continuous keys: every delta is within R_TOL, so are its means and maxima; a sum scales with the pair count
    block_keys = [k for k in ref if k.startswith("corr_mean_abs_diff_")]
    assert len(block_keys) == 6
    for k in ["corr_mean_abs_diff", "corr_rms_diff", "corr_max_abs_diff", "corr_strong_mean_abs_diff"] + block_keys:
        if np.isnan(ref[k]):                                                   # a one-column block has no pair inside it
            assert D == 6 and k == "corr_mean_abs_diff_pathways_pathways" and np.isnan(got[k])
        else:
            assert abs(got[k] - ref[k]) <= R_TOL, k
    assert abs(got["corr_frobenius_diff"] - ref["corr_frobenius_diff"]) <= R_TOL * np.sqrt(2.0 * pairs)
    if ref_stats["strong_pairs"].sum():
        share = ref_stats["strong_agree"].sum() / ref_stats["strong_pairs"].sum()
        assert abs(got["corr_strong_sign_agreement"] - share) <= 2.0 * max(left_out, 1) / ref_stats["strong_pairs"].sum()
    assert ref["corr_mean_abs_diff"] > 0.02                                    # the cohorts do differ
    # Frechet distance against double-precision moments.  Every element of a device covariance is within R_TOL sqrt(S_ii S_jj) of
    # the double one (test 3: correlations and diagonals).  The two traces then move by at most R_TOL (tr S1 + tr S2); the cross term
    # 2 tr (S1 S2)^(1/2) <= tr S1 + tr S2 is homogeneous of degree 1/2 in each covariance, so to first order the same relative
    # perturbation moves it by as much again; the means are double column sums.  Hence 2 R_TOL (tr S1 + tr S2).
    S1, S2 = Gx / (n_real - 1), Gy / (n_synth - 1)
    fref = frechet_distance(mu_x, S1, mu_y, S2)
    ftol = 2.0 * R_TOL * (np.trace(S1) + np.trace(S2))
    print(f"  frechet fp64 {fref}, tolerance {ftol:.3e}")
    for k in FRECHET_KEYS:
        assert abs(got[k] - fref[k]) <= ftol, k
    assert fref["frechet_distance"] > 100 * ftol
    np.testing.assert_allclose(mats["real_mean"], mu_x, rtol=1e-12)


@pytest.mark.parametrize("n_real,n_synth,D", E2E_CASES[1:])
def test_identical_cohorts(n_real, n_synth, D):
    x, _ = cohorts(n_real, n_synth, D)
    got = BiologicalValidator(CONF).correlation_fidelity(x, pd.DataFrame(x), frechet=True)
    assert list(got) == SUMMARY_KEYS + FRECHET_KEYS
    for k in ("corr_mean_abs_diff", "corr_rms_diff", "corr_max_abs_diff", "corr_frobenius_diff", "corr_strong_mean_abs_diff",
              "frechet_mean_term"):
        assert got[k] == 0.0, k
    assert got["corr_strong_sign_agreement"] == 1.0 and got["corr_strong_pairs"] > 0
    tr = np.trace(gram64(x)[1]) / (n_real - 1)
    assert 0.0 <= got["frechet_distance"] <= 1e-9 * tr


# ---- 6. validate_all ------------------------------------------------------------------------------------------------------------
REF_EVAL = {"evaluation": {"driver_genes": ["TP53", "RB1", "ATRX", "DLG2", "PTEN"], "mutually_exclusive_pairs": [["TP53", "MDM2"]],
                           "required_correlations": [{"mutation": "TP53", "pathway": "HALLMARK_P53_PATHWAY", "direction": "negative"},
                                                     {"mutation": "MYC", "pathway": "HALLMARK_MYC_TARGETS_V1", "direction": "positive"}]}}
CO_NAMES = ["TP53", "RB1", "ATRX", "PTEN", "MDM2", "MYC"] + [f"M{i}" for i in range(54)]
BASE_KEYS = ["mutation_frequency_correlation", "driver_gene_frequency_diff", "mutual_exclusivity_violation_rate",
             "cooccurrence_pattern_correlation", "real_pathway_coherence", "synthetic_pathway_coherence", "pathway_coherence_correlation",
             "mutation_expression_violation_rate", "ks_test_mean_pvalue", "ks_test_fraction_significant", "mmd",
             "wasserstein_distance_mean", "overall_biological_score"]
BLOCK_KEYS = [f"corr_mean_abs_diff_{a}_{b}" for a, b in (("mutations", "mutations"), ("mutations", "expression"), ("mutations", "pathways"),
                                                         ("expression", "expression"), ("expression", "pathways"), ("pathways", "pathways"))]


def test_validate_all_with_and_without_correlation(golden_dir):
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
    full = val.validate_all(*frames, correlation=True, corr_strong=0.25)
    assert [k for k in full if not k.startswith("corr_")] == BASE_KEYS
    assert [k for k in full if k.startswith("corr_")] == SUMMARY_KEYS + BLOCK_KEYS and len(full) == len(base) + 15
    for k in base:                                           # the MMD's double atomics commit in any order: last-bit freedom
        assert full[k] == pytest.approx(base[k], rel=1e-9, abs=1e-12), k
    for k, v in full.items():
        assert type(v) in (float, int), k
        f"{v:.4f}"
    real = np.concatenate([f.values for f in frames[:3]], axis=1)
    synth = np.concatenate([f.values for f in frames[3:6]], axis=1)
    alone = val.correlation_fidelity(real, synth, blocks={"mutations": 60, "expression": 40, "pathways": 2}, strong=0.25)
    assert list(alone) == SUMMARY_KEYS + BLOCK_KEYS
    for k in alone:
        assert full[k] == pytest.approx(alone[k], rel=1e-12, abs=0, nan_ok=True), k
    live = 102 - alone["corr_constant_columns"]
    assert alone["corr_pairs"] == live * (live - 1) // 2 and 0.0 <= alone["corr_max_abs_diff"] <= 2.0
    np.random.seed(123)
    both = val.validate_all(*frames, frechet=True)
    assert [k for k in both if k not in BASE_KEYS] == FRECHET_KEYS and both["frechet_distance"] >= 0.0
    assert type(both["frechet_distance"]) is float


# ---- 7. argument errors ---------------------------------------------------------------------------------------------------------
def test_boundary_arguments():
    lib = L.lib()
    x = torch.randn(40, 12, device="cuda")
    c = np.zeros(12, dtype=np.float32)
    cp = C_.c_void_p(c.ctypes.data)
    G = torch.empty((12, 12), dtype=torch.float64, device="cuda")
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gram(xp, rows, ld, D, cptr, gp):
        return lib.osd_val_centered_gram(stream, 0, xp, rows, ld, D, cptr, gp)

    assert gram(L.ptr(x), 40, 12, 12, cp, L.ptr(G)) == L.OSD_OK
    assert gram(L.ptr(x), 1, 12, 12, cp, L.ptr(G)) == L.OSD_OK                 # one row, one column: the smallest legal calls
    assert gram(L.ptr(x), 40, 12, 1, cp, L.ptr(G)) == L.OSD_OK
    assert gram(None, 40, 12, 12, cp, L.ptr(G)) == L.OSD_EINVAL
    assert gram(L.ptr(x), 40, 12, 12, None, L.ptr(G)) == L.OSD_EINVAL
    assert gram(L.ptr(x), 40, 12, 12, cp, None) == L.OSD_EINVAL
    assert gram(L.ptr(x), 0, 12, 12, cp, L.ptr(G)) == L.OSD_EINVAL
    assert gram(L.ptr(x), 40, 12, 0, cp, L.ptr(G)) == L.OSD_EINVAL
    assert gram(L.ptr(x), 40, 11, 12, cp, L.ptr(G)) == L.OSD_EINVAL
    assert b"ld >= D" in lib.osd_last_error()
    one = _kernels().centered_gram(x[:1], x[0].cpu().numpy())                  # a row against itself as centre: all zeros
    assert tuple(one.shape) == (12, 12) and not one.any()

    G2 = G.clone()
    out = (C_.c_double * (1 + 7 * 6))()

    def compare(gr, gs, D, bounds, nb, o=out):
        arr = None if bounds is None else (C_.c_int32 * len(bounds))(*bounds)
        return lib.osd_val_corr_compare(stream, 0, gr, gs, D, arr, nb, 0.3, o)

    assert compare(L.ptr(G), L.ptr(G2), 12, [0, 12], 1) == L.OSD_OK
    assert compare(L.ptr(G), L.ptr(G2), 12, [0, 5, 7, 12], 3) == L.OSD_OK
    assert compare(None, L.ptr(G2), 12, [0, 12], 1) == L.OSD_EINVAL
    assert compare(L.ptr(G), None, 12, [0, 12], 1) == L.OSD_EINVAL
    assert compare(L.ptr(G), L.ptr(G2), 12, None, 1) == L.OSD_EINVAL
    assert compare(L.ptr(G), L.ptr(G2), 12, [0, 12], 1, None) == L.OSD_EINVAL
    assert compare(L.ptr(G), L.ptr(G2), 0, [0, 0], 1) == L.OSD_EINVAL
    assert compare(L.ptr(G), L.ptr(G2), 12, [0, 12], 0) == L.OSD_EINVAL
    for bad in ([0, 7, 5, 12], [0, 5, 5, 12], [1, 5, 7, 12], [0, 5, 7, 11], [0, 5, 7, 13]):      # unsorted, empty block, wrong ends
        assert compare(L.ptr(G), L.ptr(G2), 12, bad, 3) == L.OSD_EINVAL, bad
    assert b"block bounds" in lib.osd_last_error()
    k = _kernels()
    with pytest.raises(ValueError):
        k.centered_gram(x, np.zeros(11, dtype=np.float32))
    with pytest.raises(ValueError):
        k.corr_compare(G, G2, [0, 7, 5, 12], 0.3)
    with pytest.raises(ValueError):
        k.corr_compare(G, G2.float(), [0, 12], 0.3)
    val = BiologicalValidator(CONF)
    good = np.ones((9, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="same features"):
        val.correlation_fidelity(good, good[:, :7])
    with pytest.raises(ValueError, match="at least 2"):
        val.correlation_fidelity(good, good[:1])
    bad = good.copy()
    bad[2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        val.correlation_fidelity(bad, good)
    bad[2, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        val.correlation_fidelity(good, bad)
    allconst = val.correlation_fidelity(good, good)                            # every column constant: no pair, NaN means, no error
    assert allconst["corr_pairs"] == 0 and allconst["corr_constant_columns"] == 8 and np.isnan(allconst["corr_mean_abs_diff"])
