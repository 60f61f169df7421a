"""GPU: ``osd_val_group_ranks`` (csrc/diffexp.hip: col_tiles<true>, the segmented sort, de_stats, de_finish), and
``BiologicalValidator.differential_fidelity`` above it, against the int64 / float64 restatement of tests/diffexp_helpers.py evaluated
on the same fp32 inputs.

Kernel shapes (na, nb, D): (1, 1, 1), (1, 7, 5), (5, 3, 6), (64, 65, 33), (257, 130, 130) -- small, row tails, column counts off the
wavefront width; (130, 4099, 66) many controls per case value and (4099, 130, 5) the reverse; (4097, 8193, 3) a segment over two
SEG_CHUNKs; (20001, 30011, 8) windows beyond the LDS stage of 4096 values (on a binary or a signed-zero column a run that crosses from
one value to the next asks for every equal value of the other group: 13 500 ones, 24 000 zeros).  Each runs dense with the cases and
the controls in blocks, alternating, and alternating with ignored rows (labels -1 and 2, values 1000) in between, and as an aligned and
as an unaligned column slice of a wider matrix full of 1000s, on seven kinds of data (diffexp_helpers.KINDS).

  * u2, ties, na, nb EQUAL the int64 restatement; all-equal data: u2 = na nb and ties = N^3 - N; disjoint supports: u2 = 0 or 2 na nb;
    the labels swapped: u2' = 2 na nb - u2, the same ties, the groups' moments exchanged bit for bit;
  * moments: |sum - ref| <= (n + 4) 2^-52 sum |x - c| and |sumsq - ref| <= (n + 4) 2^-52 sum (x - c)^2, n the group's size: one
    rounding each for the difference and the square, n roundings in the sum; integer data: exact;
  * chunk_cols 0, 1, 7 and D, a repeated call and a permutation of the rows: identical bits; bad arguments: OSD_EINVAL.

End to end (600 real, 900 synthetic, D = 130 in three blocks, a binary and a continuous contrast): every summary key -- each derives
from the integers u2 and ties -- EQUALS the float64 pipeline (the package's own host code over the NumPy stand-in), and so do the
per-feature AUC, effect, z, p and q; the moment-derived rows (mean difference, Welch t, Cohen's d) are held to it.
    Measured, the largest |device - float64| / |float64| over those rows of both cohorts and contrasts: faithful 3.217e-15,
    exaggerating 2.611e-15 (the same figures on a second run: the kernel's bits do not change) -- the device's moment sums, double sums
    in another order than NumPy's, are the whole of it.
    Asserted: 4 x the largest."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import diffexp as DE
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels
from diffexp_helpers import INTEGER_KINDS, KINDS, U52, NumpyKernels, arrange, group_ranks64, make_groups, planted_cohort

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 5), (5, 3, 6), (64, 65, 33), (257, 130, 130), (130, 4099, 66), (4099, 130, 5), (4097, 8193, 3), (20001, 30011, 8)]
VARIANTS = [("dense", "blocks"), ("dense", "alternating"), ("dense", "ignored"), ("slice_aligned", "alternating"), ("slice_unaligned", "ignored")]
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
def _case(kind, na, nb, D):
    """The groups, the centre (an integer on integer data, so that the moments stay exact; else the fp32 column means) and the
    restatement, which no arrangement of the rows changes."""
    a, b = make_groups(kind, na, nb, D)
    center = np.full(D, 1.0, dtype=np.float32) if kind in INTEGER_KINDS else np.concatenate([a, b]).mean(0).astype(np.float32)
    x, labels = arrange(a, b, "blocks")
    return a, b, center, group_ranks64(x, labels, center)


def _check(got, ref, kind, na, nb, D):
    n = na + nb
    assert (got["na"], got["nb"]) == (na, nb) == (ref["na"], ref["nb"])
    for name in ("u2", "ties"):
        assert got[name].dtype == np.int64 and got[name].shape == (D,)
        assert np.array_equal(got[name], ref[name]), (name, int((got[name] != ref[name]).sum()), D)
    worst = 0.0
    for name, scale in (("sum", ref["sum_abs"]), ("sumsq", ref["sumsq"])):
        assert got[name].dtype == np.float64 and got[name].shape == (2, D) and np.isfinite(got[name]).all()
        if kind in INTEGER_KINDS:
            assert np.array_equal(got[name], ref[name]), name
        bound = (np.array([[na], [nb]]) + 4) * U52 * scale
        err = np.abs(got[name] - ref[name])
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, worst)
    if kind == "all_equal":
        assert (got["u2"] == na * nb).all() and (got["ties"] == n ** 3 - n).all()
    if kind == "disjoint":
        assert (got["u2"][0::2] == 2 * na * nb).all() and (got["u2"][1::2] == 0).all()
    return worst


@pytest.mark.parametrize("layout,how", VARIANTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na,nb,D", SHAPES)
def test_group_ranks_against_restatement(na, nb, D, kind, layout, how):
    a, b, center, ref = _case(kind, na, nb, D)
    x, labels = arrange(a, b, how)
    got = _kernels().group_ranks(_layout(x, layout), _t(labels), center)
    worst = _check(got, ref, kind, na, nb, D)
    print(f"group_ranks {na}x{nb}x{D} {kind} {layout} {how}: max moment err / bound {worst:.3g}")


@pytest.mark.parametrize("kind", ["continuous", "zero_inflated", "signed_zeros"])
@pytest.mark.parametrize("na,nb,D", SHAPES)
def test_group_ranks_swapped_labels_and_no_center(na, nb, D, kind):
    a, b, _, _ = _case(kind, na, nb, D)
    x, labels = arrange(a, b, "ignored")
    k, xd = _kernels(), _t(x)
    got = k.group_ranks(xd, _t(labels))
    ref = group_ranks64(x, labels)
    _check(got, ref, kind, na, nb, D)
    swapped = k.group_ranks(xd, _t(np.where(labels == 1, 0, np.where(labels == 0, 1, labels)).astype(np.int32)))
    assert (swapped["na"], swapped["nb"]) == (nb, na)
    assert np.array_equal(swapped["u2"], 2 * na * nb - got["u2"]) and np.array_equal(swapped["ties"], got["ties"])
    for name in ("sum", "sumsq"):                              # a group's sums run over its own sorted segment: the same partition
        assert np.array_equal(swapped[name][::-1].view(np.int64), got[name].view(np.int64)), name


@pytest.mark.parametrize("kind", ["continuous", "zero_inflated"])
@pytest.mark.parametrize("na,nb,D", SHAPES)
def test_group_ranks_same_bits_at_every_chunk_and_row_order(na, nb, D, kind):
    a, b, center, _ = _case(kind, na, nb, D)
    x, labels = arrange(a, b, "ignored")
    k, xd, ld = _kernels(), _t(x), _t(labels)
    first = k.group_ranks(xd, ld, center)

    def same(again, what):
        for name in ("u2", "ties"):
            assert np.array_equal(again[name], first[name]), (name, what)
        for name in ("sum", "sumsq"):
            assert np.array_equal(again[name].view(np.int64), first[name].view(np.int64)), (name, what)
        assert (again["na"], again["nb"]) == (na, nb)

    for chunk in (0, 1, 7, D):
        same(k.group_ranks(xd, ld, center, chunk_cols=chunk), chunk)
    perm = np.random.default_rng(na + nb).permutation(x.shape[0])
    same(k.group_ranks(_t(x[perm]), _t(labels[perm]), center), "permuted")
    same(k.group_ranks(_t(x[::-1]), _t(labels[::-1]), center, chunk_cols=7), "reversed")
    timed = k.group_ranks(xd, ld, center, chunk_cols=7, phases=True)
    same(timed, "timed")
    assert timed["phase_ms"].shape == (3,) and (timed["phase_ms"] >= 0).all() and timed["phase_ms"].sum() > 0


def test_group_ranks_argument_errors():
    lib = L.lib()
    x = torch.zeros((8, 8), device="cuda")
    lab = torch.tensor([1, 0, 1, 0, -1, 2, 1, 0], dtype=torch.int32, device="cuda")
    out = [np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64), np.zeros(16), np.zeros(16), np.zeros(1, dtype=np.int64),
           np.zeros(1, dtype=np.int64)]
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(X=x, rows=8, ld=8, D=8, labels=lab, center=None, chunk=0, drop=None):
        ptrs = [None if i == drop else C_.c_void_p(o.ctypes.data) for i, o in enumerate(out)]
        return lib.osd_val_group_ranks(stream, 0, L.ptr(X), rows, ld, D, L.ptr(labels), L.ptr(center), chunk, *ptrs)

    assert call() == L.OSD_OK and (int(out[4][0]), int(out[5][0])) == (3, 3)
    assert call(chunk=3) == L.OSD_OK and call(chunk=1000) == L.OSD_OK and call(D=4) == L.OSD_OK and call(center=x[0].contiguous()) == L.OSD_OK
    no_case, no_control = torch.where(lab == 1, 5, lab).to(torch.int32), torch.where(lab == 0, -7, lab).to(torch.int32)
    for bad in [dict(X=None), dict(labels=None), dict(rows=0), dict(rows=-1), dict(D=0), dict(D=-2), dict(ld=7), dict(chunk=-1),
                dict(labels=no_case), dict(labels=no_control)] + [dict(drop=i) for i in range(6)]:
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error()
    # more than 2^20 labelled rows: one column, refused after the labels are counted
    rows = (1 << 20) + 1
    big, many = torch.zeros((rows, 1), device="cuda"), torch.ones(rows, dtype=torch.int32, device="cuda")
    many[::2] = 0
    assert call(X=big, rows=rows, ld=1, D=1, labels=many) == L.OSD_EINVAL and "2^20" in L.last_error()
    many[0] = 3                                               # 2^20 labelled rows pass
    assert call(X=big, rows=rows, ld=1, D=1, labels=many) == L.OSD_OK and int(out[4][0]) + int(out[5][0]) == 1 << 20
    assert out[0][0] == (1 << 19) * (1 << 19) and out[1][0] == (1 << 60) - (1 << 20)
    k = _kernels()
    with pytest.raises(ValueError):
        k.group_ranks(x, lab[:7])
    with pytest.raises(ValueError):
        k.group_ranks(x, lab, chunk_cols=-1)
    with pytest.raises(ValueError):
        k.group_ranks(x, lab, center=np.zeros(7))
    with pytest.raises(ValueError):
        k.group_ranks(x, no_case)


# ---- 2. differential_fidelity end to end ------------------------------------------------------------------------------------------
N_REAL, N_SYNTH = 600, 900
BLOCKS = {"mutations": 20, "expression": 90, "pathways": 20}
WIDTHS = (20, 90, 20)
E2E_D = 130
NAMES = ["metastasis", "age"]
MOMENT_ROWS = ("mean_diff", "welch_t", "cohen_d")
E2E_OBSERVED = 3.217e-15         # measured max |device - float64| / |float64| over the moment-derived rows of the two samplers
E2E_TOL = 4 * E2E_OBSERVED


SAMPLERS = {"faithful": 1.0, "exaggerating": 2.0}            # how strongly the synthetic cohort follows its conditions


@functools.lru_cache(maxsize=None)
def _cohorts(sampler="exaggerating"):
    return planted_cohort(N_REAL, 11, WIDTHS), planted_cohort(N_SYNTH, 12, WIDTHS, scale=SAMPLERS[sampler])


@functools.lru_cache(maxsize=None)
def _pipeline64(sampler):
    """The float64 pipeline: the package's own host code over the float64 kernels."""
    (x, cr), (y, cs) = _cohorts(sampler)
    return DE.differential_metrics(NumpyKernels(), torch.from_numpy(x), cr, torch.from_numpy(y), cs, NAMES, [0, 20, 110, 130], list(BLOCKS))


@functools.lru_cache(maxsize=None)
def _device(sampler="exaggerating"):
    (x, cr), (y, cs) = _cohorts(sampler)
    return BiologicalValidator(CONF).differential_fidelity(x, cr, y, cs, names=NAMES, blocks=BLOCKS, return_rows=True)


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_differential_fidelity_equals_float64_pipeline(sampler):
    (got, rows), (want, rows64) = _device(sampler), _pipeline64(sampler)
    assert list(got) == list(want) and got["de_contrasts"] == 2 and got["de_skipped"] == 0
    for key, w in want.items():
        assert got[key] == w or (np.isnan(got[key]) and np.isnan(w)), (key, got[key], w)
    worst = 0.0
    for name in NAMES:
        assert (rows[name]["threshold"] is None) == (name == "metastasis") and rows[name]["threshold"] == rows64[name]["threshold"]
        for cohort in ("real", "synthetic"):
            d, h = rows[name][cohort], rows64[name][cohort]
            assert (d["na"], d["nb"]) == (h["na"], h["nb"]) and d["na"] + d["nb"] == (N_REAL if cohort == "real" else N_SYNTH)
            for field in ("u2", "ties", "auc", "effect", "z", "p", "q"):
                assert np.array_equal(d[field], h[field]), (name, cohort, field)
            for field in MOMENT_ROWS:
                assert d[field].shape == (E2E_D,) and np.isfinite(d[field]).all()
                worst = max(worst, float(np.max(np.abs(d[field] - h[field]) / np.abs(h[field]))))
    print(f"differential_fidelity {sampler}: largest |device - float64| / |float64| over the moment-derived rows = {worst:.3e}")
    assert worst <= E2E_TOL, worst


def test_differential_fidelity_reads_the_planted_signal():
    """Float64 pipeline, binary contrast: effect_slope 0.710 (faithful) and 1.292 (exaggerating), recall 0.667 and 0.952, sign
    agreement 0.952 both; the device figures equal them (the test above)."""
    faithful, strong = _device("faithful")[0], _device("exaggerating")[0]
    # a synthetic cohort that follows its conditions twice as strongly: a steeper slope on both contrasts, the same signs
    assert strong["de_effect_slope_metastasis"] > faithful["de_effect_slope_metastasis"] + 0.25
    assert strong["de_effect_slope_age"] > faithful["de_effect_slope_age"] + 0.2
    assert strong["de_sign_agreement_metastasis"] > 0.9 and faithful["de_sign_agreement_metastasis"] > 0.9
    assert strong["de_real_hits_metastasis"] == faithful["de_real_hits_metastasis"] >= 15
    assert 0 <= strong["de_max_gap_feature_metastasis"] < E2E_D and f"{strong['de_max_gap_feature_metastasis']:.4f}"


def test_validate_all_carries_the_differential_keys():
    import pandas as pd
    (x, cr), (y, cs) = _cohorts()

    def frames(a):
        mut = pd.DataFrame(a[:, :20], columns=[f"M{i}" for i in range(20)])
        expr = pd.DataFrame(a[:, 20:110], columns=[f"G{i}" for i in range(90)])
        pw = pd.DataFrame(a[:, 110:], columns=[f"PW{i}" for i in range(20)])
        return mut, expr, pw

    val = BiologicalValidator(CONF)
    np.random.seed(5)
    plain = val.validate_all(*frames(x), *frames(y))
    np.random.seed(5)
    full = val.validate_all(*frames(x), *frames(y), differential=(cr, cs), differential_names=NAMES)
    assert not any(k.startswith("de_") for k in plain)
    extra = [k for k in full if k not in plain]
    assert all(k.startswith("de_") for k in extra) and [k for k in full if k in plain] == list(plain)
    assert all(full[k] == pytest.approx(plain[k], rel=1e-9, abs=1e-12, nan_ok=True) for k in plain)      # double atomics: last-bit freedom
    direct = _device()[0]
    assert extra == list(direct) and all(full[k] == direct[k] or (np.isnan(full[k]) and np.isnan(direct[k])) for k in extra)
    named = val.validate_all(*frames(x), *frames(y), differential=(pd.DataFrame(cr, columns=NAMES), cs))
    assert [k for k in named if k.startswith("de_")] == extra
    with pytest.raises(ValueError):
        val.validate_all(*frames(x), *frames(y), differential=(cr,))


def test_differential_fidelity_argument_errors_and_shards():
    (x, cr), (y, cs) = _cohorts()
    val = BiologicalValidator(CONF)
    bad = np.array(x)
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match="real"):
        val.differential_fidelity(bad, cr, y, cs)
    with pytest.raises(ValueError, match="synthetic"):
        val.differential_fidelity(x, cr, y[:, :100], cs)
    with pytest.raises(ValueError, match="synthetic"):
        val.differential_fidelity(x, cr, y, cs[:-1])
    with pytest.raises(ValueError):
        val.differential_fidelity(x, cr, y, cs, names=["only_one"])
    with pytest.raises(ValueError):
        val.differential_fidelity(x, cr, y, cs, blocks={"a": 100, "b": 20})
    with pytest.raises(ValueError):
        val.differential_fidelity(x, cr, y, cs, alpha=0.0)
    skipped = val.differential_fidelity(x, cr, y, np.column_stack([np.ones(N_SYNTH), cs[:, 1]]), names=NAMES)
    assert skipped["de_skipped"] == 1 and skipped["de_contrasts"] == 1 and "de_recall_age" in skipped and "de_recall_metastasis" not in skipped
    sharded = BiologicalValidator(CONF, sharded=True)
    with pytest.raises(ValueError, match="shard"):
        sharded.differential_fidelity(x, cr, y, cs)
