"""GPU: ``osd_val_pathway_scores`` and ``osd_val_pathway_agreement`` (csrc/pathway.hip: pw_linear, pw_ssgsea, pa_partial),
``pathways.PathwayScorer`` and ``BiologicalValidator.pathway_consistency`` above them, against the float64 restatement of
tests/pathway_helpers.py.

Kernel shapes (D; set sizes), rows 1, 3 and 67: (2; 1), (5; 1, 4), (64; 1, 63), (65; 2, 64), (257; 5, 255, 256) -- the smallest rows,
sets of one and of all but one gene, sizes around the wavefront width and the workgroup's trip counts; (1025; 1 ... 1024) a row just
above a power of two whose sets use every gene; (5054; 29 overlapping sets of 5 ... 200, one listed twice) the reference's width;
(32768; 1024, 7, 1) and (32768; 32 sets of 1024 that use every gene), 3 rows: the largest row, 128 KiB of keys.  Each with ld = D
and with ld = D + 62 from a base 62 floats into a buffer whose other floats are NaN.  Six kinds of rows: continuous; 30 % zeros with
a -0.0 among them; all values equal (every mid-rank (D + 1) / 2); integers 0 ... 3; one +inf and one -inf per row; one row with a NaN.

  * ssgsea within 8 (m + 4) 2^-53 D of the restatement: the integer ranks are exact and the table is shared, m products and 2 m
    additions on either side, each result at most D; a NaN row is all NaN and its neighbours are untouched;
  * mean and zscore within 2 (m + 4) 2^-53 norm sum_j |(x_j - c_j) s_j|; where the restatement is not finite the kernel gives the
    same inf or NaN;
  * the agreement sums within (rows + 4) 2^-53 sum |term| of float64 sums over the same doubles, the used-row counts equal;
  * row_chunk 0, 1, 7 and rows, a repeated call and the timed twin: identical bits; permuted rows permute the outputs; the set listed
    twice has equal bits;
  * a zero-inflated row with a -0.0, its columns shuffled and the members renamed with them: identical bits in all three methods;
  * column slices of one combined device matrix reach the kernels in place and give the figures of contiguous copies;
  * every OSD_EINVAL case, D = 32768 passes and D = 32769 is refused; the wrapper's ValueErrors.

End to end (600 real and 900 synthetic patients, 90 genes, seven sets, seed 7; mean and ssgsea): every ``pwc_*`` key within 1e-9 of
the float64 pipeline -- the package's own host code over the NumPy stand-in.  A score differs from the restatement by at most
8 * 93 * 2^-53 * 90 < 1e-11, the standardisation multiplies it by 1 / sd < 10 here, and every figure is a mean or a ratio of such
values over 900 rows at a condition number below 100 -- and the faithful / decoupled assertions of the CPU test on the device values."""
import ctypes as C_
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import pathways as PW
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceFrame, DeviceKernels
from pathway_helpers import (KINDS, N_GENES, N_SYNTH, U53, NumpyKernels, agreement64, covering_sets, linear64, make_rows, make_sets,
                             planted_cohorts, rank_table, ssgsea64)

pytestmark = pytest.mark.gpu

PAD = 62                                                       # the expression block starts 62 floats into the combined matrix
CONF = {"evaluation": {}}
SHAPES = {
    "d2": (2, (1,), (1, 3, 67)),
    "d5": (5, (1, 4), (1, 3, 67)),
    "d64": (64, (1, 63), (1, 3, 67)),
    "d65": (65, (2, 64), (1, 3, 67)),
    "d257": (257, (5, 255, 256), (1, 3, 67)),
    "d1025": (1025, (1, 2, 63, 64, 65, 255, 256, 257, 1024), (1, 3, 67)),
    "d5054": (5054, None, (1, 3, 67)),
    "d32768": (32768, (1024, 7, 1), (3,)),
    "d32768_every_gene": (32768, None, (3,)),
}


def _kernels():
    return DeviceKernels(torch.device("cuda", torch.cuda.current_device()))


@functools.lru_cache(maxsize=None)
def _sets(name):
    D, sizes, _ = SHAPES[name]
    rs = np.random.default_rng(D)
    if name == "d5054":                                        # a pool of 700 genes: the sets overlap heavily; set 3 comes twice
        pool = rs.choice(D, 700, replace=False)
        sets = [rs.choice(pool, int(m), replace=False) for m in np.linspace(5, 200, 28).astype(int)]
        return sets + [sets[3].copy()]
    if name == "d32768_every_gene":
        sets = covering_sets(D, 1024)
        assert len(sets) == 32 and np.unique(np.concatenate(sets)).size == D
        return sets
    if name == "d1025":                                        # the set of 1024 and the set of 1 use every gene between them: U = D
        perm = rs.permutation(D)
        sets = [perm[1024:]] + make_sets(D, sizes[1:-1]) + [perm[:1024]]
        assert np.unique(np.concatenate(sets)).size == D
        return sets
    return make_sets(D, sizes)


def _place(x, ld_extra):
    """x on the device as a [rows, D] view with the row stride D + ld_extra, PAD floats into a buffer of NaNs when ld_extra > 0."""
    t = torch.from_numpy(x).cuda()
    if not ld_extra:
        return t
    rows, D = x.shape
    ld = D + ld_extra
    buf = torch.full((PAD + rows * ld,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[PAD:].view(rows, ld)[:, :D]
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + 4 * PAD and (rows == 1 or view.stride(0) == ld)
    return view


def _center_scale(D):
    rs = np.random.default_rng(D + 1)
    c, s = rs.standard_normal(D).astype(np.float32), (0.2 + rs.random(D)).astype(np.float32)
    s[::7] = 0.0                                               # a constant gene of the cohort: scale 0
    return c, s


def _check_close(got, want, bound, what):
    """Within the bound where the restatement and its bound are finite, the same inf or NaN elsewhere."""
    finite = np.isfinite(want) & np.isfinite(bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    worst = float(np.max(np.where(finite, err / np.maximum(bound, 1e-300), 0.0))) if finite.any() else 0.0
    print(f"{what}: largest error / bound {worst:.3f}")
    assert (err[finite] <= bound[finite]).all(), what
    assert np.array_equal(got[~finite], want[~finite], equal_nan=True), what


# ---- 1. the scoring kernels against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_scores_equal_the_restatement(name, kind):
    D, _, row_counts = SHAPES[name]
    sets = _sets(name)
    sizes = np.array([len(m) for m in sets], dtype=np.float64)
    table = rank_table(D)
    c, s = _center_scale(D)
    k = _kernels()
    for rows in row_counts:
        x = make_rows(kind, rows, D)
        want = {"ssgsea": ssgsea64(x, sets, table), "mean": linear64(x, sets, "mean"), "zscore": linear64(x, sets, "zscore", c, s)}
        for ld_extra in (0, PAD):
            t = _place(x, ld_extra)
            what = f"{name} {kind} rows={rows} ld=D+{ld_extra}"
            got = k.pathway_scores(t, sets, "ssgsea", rank_table=table).cpu().numpy()
            assert got.shape == (rows, len(sets))
            _check_close(got, want["ssgsea"], np.broadcast_to(8 * (sizes + 4) * U53 * D, got.shape), what + " ssgsea")
            if kind == "nan_row":
                bad = np.isnan(x).any(axis=1)
                assert bad.sum() == 1 and np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
            if kind == "all_equal":                            # every mid-rank is (D + 1) / 2: the two terms cancel up to rounding
                assert (np.abs(got) <= 8 * (sizes + 4) * U53 * D).all()
            for method, args in (("mean", {}), ("zscore", dict(center=c, scale=s))):
                got = k.pathway_scores(t, sets, method, **args).cpu().numpy()
                ref, mag = want[method]
                _check_close(got, ref, 2 * (sizes + 4) * U53 * mag, what + " " + method)


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_ssgsea_other_exponents(alpha):
    D = 257
    sets, x = _sets("d257"), make_rows("zero_inflated", 5, 257)
    table = rank_table(D, alpha)
    got = _kernels().pathway_scores(torch.from_numpy(x).cuda(), sets, "ssgsea", rank_table=table).cpu().numpy()
    sizes = np.array([len(m) for m in sets], dtype=np.float64)
    _check_close(got, ssgsea64(x, sets, table), np.broadcast_to(8 * (sizes + 4) * U53 * D, got.shape), f"alpha={alpha}")


# ---- 2. reproducibility -------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("method", ["mean", "zscore", "ssgsea"])
@pytest.mark.parametrize("name,kind", [("d5054", "zero_inflated"), ("d1025", "nan_row"), ("d65", "integers")])
def test_the_same_bits_at_every_chunk_and_row_order(name, kind, method):
    D, rows = SHAPES[name][0], 67
    sets, x = _sets(name), make_rows(kind, rows, D)
    c, s = _center_scale(D)
    args = {"mean": {}, "zscore": dict(center=c, scale=s), "ssgsea": dict(rank_table=rank_table(D))}[method]
    k, t = _kernels(), _place(x, PAD)
    first = _bits(k.pathway_scores(t, sets, method, **args))
    for chunk in (0, 1, 7, rows, rows + 1):
        assert np.array_equal(_bits(k.pathway_scores(t, sets, method, row_chunk=chunk, **args)), first), chunk
    assert np.array_equal(_bits(k.pathway_scores(t, sets, method, **args)), first)
    timed, ms = k.pathway_scores(t, sets, method, row_chunk=7, phases=True, **args)
    assert np.array_equal(_bits(timed), first) and ms.shape == (2,) and (ms >= 0).all() and ms.sum() > 0
    perm = np.random.default_rng(2).permutation(rows)
    assert np.array_equal(_bits(k.pathway_scores(torch.from_numpy(x[perm]).cuda(), sets, method, **args)), first[perm])
    if name == "d5054":
        assert np.array_equal(first[:, 3], first[:, 28])       # the set listed twice


@pytest.mark.parametrize("D", [300, 5054])
def test_ties_do_not_depend_on_where_equal_values_sit(D):
    """Zero-inflated rows with a -0.0 among the zeros, their columns shuffled (the members renamed with them, in the same listing
    order): every member keeps its mid-rank, so all three methods give the same bits -- the device's tie handling, not the
    restatement's, is what this holds."""
    rows = 5
    x = make_rows("zero_inflated", rows, D)
    assert np.signbit(x).sum() == rows and ((x == 0).sum(axis=1) > D // 5).all()
    rs = np.random.default_rng(D)
    sets = [rs.permutation(D)[:m] for m in (5, 40, 200, min(D - 1, 1024))]
    c, s = _center_scale(D)
    table = rank_table(D)
    k = _kernels()
    for trial in range(3):
        perm = rs.permutation(D)
        inv = np.empty(D, dtype=np.int64)
        inv[perm] = np.arange(D)
        moved_sets = [inv[m] for m in sets]
        for method, args, moved_args in (("ssgsea", dict(rank_table=table), dict(rank_table=table)), ("mean", {}, {}),
                                         ("zscore", dict(center=c, scale=s), dict(center=c[perm], scale=s[perm]))):
            base = _bits(k.pathway_scores(torch.from_numpy(x).cuda(), sets, method, **args))
            moved = _bits(k.pathway_scores(torch.from_numpy(np.ascontiguousarray(x[:, perm])).cuda(), moved_sets, method, **moved_args))
            assert np.array_equal(base, moved), (method, trial)


# ---- 3. the agreement sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,S", [(1, 1), (3, 7), (67, 26), (4097, 3), (9000, 26)])
def test_agreement_sums_equal_the_restatement(rows, S):
    rs = np.random.default_rng(rows + S)
    scores = rs.standard_normal((rows, S)) * 3.0 + 5.0
    block = rs.standard_normal((rows, S + 5)).astype(np.float32)
    if rows > 2:                                               # rows that a pathway leaves out: a non-finite z or g
        scores[1, 0], scores[rows // 2, S - 1] = np.nan, np.inf
        block[2, 0], block[rows - 1, S // 2] = np.inf, np.nan
    mu, isd = rs.standard_normal(S) + 5.0, 1.0 / (2.0 + rs.random(S))
    k = _kernels()
    p = torch.from_numpy(scores).cuda()
    want, used, mag = agreement64(scores, block, mu, isd)
    for g in (torch.from_numpy(np.ascontiguousarray(block[:, :S])).cuda(), torch.from_numpy(block).cuda()[:, :S]):
        got = k.pathway_agreement(p, g, mu, isd)
        assert got["sums"].shape == (S, 6) and got["used"].dtype == np.int64 and np.array_equal(got["used"], used)
        err = np.abs(got["sums"] - want)
        print(f"rows={rows} S={S}: largest error / bound {np.max(err / np.maximum((rows + 4) * U53 * mag, 1e-300)):.3f}")
        assert (err <= (rows + 4) * U53 * mag).all()
        again = k.pathway_agreement(p, g, mu, isd)
        assert np.array_equal(again["sums"].view(np.int64), got["sums"].view(np.int64)) and np.array_equal(again["used"], used)
    if rows > 2:
        assert used[0] == rows - 2 and (used <= rows).all() and used.min() >= rows - 2


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = L.lib()
    D, S, rows = 16, 2, 4
    x = torch.rand(rows, D, device="cuda")
    cs = torch.ones(D, device="cuda")
    out = torch.zeros(rows, S, dtype=torch.float64, device="cuda")
    off, mem = np.array([0, 3, 8], dtype=np.int32), np.array([0, 5, 9, 1, 2, 3, 4, 15], dtype=np.int32)
    table = rank_table(D)
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def hp(a):
        return None if a is None else C_.c_void_p(a.ctypes.data)

    def dp(t):
        return None if t is None else C_.c_void_p(t.data_ptr())

    def call(x=x, rows=rows, ld=D, D=D, method=2, c=None, s=None, off=off, mem=mem, S=S, table=table, chunk=0, out=out, timed=None):
        args = [stream, 0, dp(x), rows, ld, D, method, dp(c), dp(s), hp(off), hp(mem), S, hp(table), chunk, dp(out)]
        if timed is not None:
            return lib.osd_val_pathway_scores_timed(*args, timed[0])
        return lib.osd_val_pathway_scores(*args)

    def arr(v):
        return np.array(v, dtype=np.int32)

    assert call() == L.OSD_OK and call(chunk=3) == L.OSD_OK and call(method=0, table=None) == L.OSD_OK
    assert call(method=1, c=cs, s=cs, table=None) == L.OSD_OK and call(method=1, table=None) == L.OSD_OK
    ms = (C_.c_float * 2)()
    assert call(timed=[ms]) == L.OSD_OK and all(v >= 0 for v in ms)
    assert call(off=arr([0, 15]), mem=arr(np.arange(15)), S=1) == L.OSD_OK                  # m = D - 1 passes, m = D does not
    cases = [dict(x=None), dict(off=None), dict(mem=None), dict(out=None), dict(table=None), dict(timed=[None]),
             dict(method=3), dict(method=-1), dict(D=1), dict(D=0), dict(rows=0), dict(rows=-2), dict(ld=15), dict(S=0), dict(S=-1),
             dict(chunk=-1),
             dict(off=arr([0, 0, 8])), dict(off=arr([0, 8, 3])), dict(off=arr([1, 3, 8])),                 # an empty set, m < 0, a start off 0
             dict(off=arr([0, 16]), mem=arr(np.arange(16)), S=1),                                              # m == D
             dict(mem=arr([0, 5, 16, 1, 2, 3, 4, 15])), dict(mem=arr([0, 5, -1, 1, 2, 3, 4, 15])),            # outside [0, D)
             dict(mem=arr([0, 5, 5, 1, 2, 3, 4, 15])), dict(mem=arr([0, 5, 9, 1, 2, 3, 1, 15]))]              # repeated inside a set
    for bad in cases:
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error(), bad
    assert call(mem=arr([0, 5, 9, 0, 5, 9, 4, 15])) == L.OSD_OK                             # the same gene in two sets is no repeat
    wide = torch.rand(2, 2000, device="cuda")
    assert call(x=wide, rows=2, ld=2000, D=2000, off=arr([0, 1025]), mem=arr(np.arange(1025)), S=1, table=rank_table(2000)) == L.OSD_EINVAL
    assert "1024" in L.last_error()
    assert call(x=wide, rows=2, ld=2000, D=2000, off=arr([0, 1024]), mem=arr(np.arange(1025)), S=1, table=rank_table(2000)) == L.OSD_OK
    big, one = torch.rand(1, 32769, device="cuda"), arr([32767])
    small_out = torch.zeros(1, 1, dtype=torch.float64, device="cuda")
    assert call(x=big, rows=1, ld=32769, D=32768, off=arr([0, 1]), mem=one, S=1, table=rank_table(32768), out=small_out) == L.OSD_OK
    assert call(x=big, rows=1, ld=32769, D=32769, off=arr([0, 1]), mem=one, S=1, table=rank_table(32769), out=small_out) == L.OSD_EINVAL
    assert "32768" in L.last_error()

    scores = torch.zeros(rows, S, dtype=torch.float64, device="cuda")
    block = torch.zeros(rows, S, device="cuda")
    mu, sums, used = np.zeros(S), np.zeros((S, 6)), np.zeros(S, dtype=np.int64)

    def agree(scores=scores, rows=rows, S=S, block=block, ld_b=S, mu=mu, isd=mu, sums=sums, used=used):
        return lib.osd_val_pathway_agreement(stream, 0, dp(scores), rows, S, dp(block), ld_b, hp(mu), hp(isd), hp(sums), hp(used))

    assert agree() == L.OSD_OK and used.tolist() == [rows] * S
    for bad in [dict(scores=None), dict(block=None), dict(mu=None), dict(isd=None), dict(sums=None), dict(used=None), dict(rows=0),
                dict(S=0), dict(S=65536), dict(ld_b=S - 1)]:
        assert agree(**bad) == L.OSD_EINVAL, bad
        assert L.last_error(), bad

    k = _kernels()
    good = [[0, 5, 9], [1, 2, 3, 4, 15]]
    assert tuple(k.pathway_scores(x, good, "ssgsea", rank_table=table).shape) == (rows, 2)
    for bad in [dict(sets=[]), dict(row_chunk=-1), dict(method="gsva"), dict(rank_table=None), dict(rank_table=table[:-1]),
                dict(sets=[[0, 16]]), dict(sets=[[3, 3]]), dict(sets=[[]]), dict(sets=[list(range(16))]), dict(sets=[[2 ** 40]]),
                dict(t=x[:, :1], sets=[[0]]), dict(method="zscore", center=np.ones(3))]:
        args = dict(t=x, sets=good, method="ssgsea", rank_table=table)
        args.update(bad)
        with pytest.raises(ValueError):
            k.pathway_scores(**args)
    for bad in [dict(scores=scores.float()), dict(block=block[:, :1]), dict(block=block[:2]), dict(mu=np.zeros(3))]:
        args = dict(scores=scores, block=block, mu=mu, isd=mu)
        args.update(bad)
        with pytest.raises(ValueError):
            k.pathway_agreement(**args)


# ---- 5. the scorer and pathway_consistency end to end ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cohorts(method):
    return planted_cohorts(method)


@functools.lru_cache(maxsize=None)
def _pipeline64(method, block):
    c = _cohorts(method)
    return PW.pathway_consistency(ShardComm(False), NumpyKernels(), "cpu", c["synth"], c[block], c["sets"], c["real"], c["real_block"],
                                  method=method)


@functools.lru_cache(maxsize=None)
def _device(method, block):
    c = _cohorts(method)
    return BiologicalValidator(CONF).pathway_consistency(c["synth"], c[block], c["sets"], c["real"], c["real_block"], method=method,
                                                         return_rows=True)


@pytest.mark.parametrize("block", ["faithful", "decoupled"])
@pytest.mark.parametrize("method", ["mean", "ssgsea"])
def test_pathway_consistency_equals_float64_pipeline(method, block):
    (got, rows), (want, rows64) = _device(method, block), _pipeline64(method, block)
    assert list(got) == list(want) and rows["names"] == rows64["names"] == _cohorts(method)["names"]
    names = rows["names"]
    for key, w in want.items():
        if key.endswith("_pathway"):                           # the pathway a figure names attains the float64 extreme (the real cohort's
            cohort = "real" if key.startswith("pwc_real_") else "synthetic"       # r are all 1 up to rounding: any of them may be named)
            field = "pearson" if "pearson" in key else "rmse"
            assert abs(rows64[cohort][field][names.index(got[key])] - want[key[:-len("_pathway")]]) <= 1e-9, (key, got[key], w)
        elif isinstance(w, (str, int)):
            assert got[key] == w, (key, got[key], w)
        else:
            print(f"{method} {block} {key}: device {got[key]!r} float64 {w!r}")
            assert abs(got[key] - w) <= 1e-9, (key, got[key], w)
    for cohort in ("synthetic", "real"):
        assert np.array_equal(rows[cohort]["n"], rows64[cohort]["n"])
        for field in ("pearson", "rmse", "bias", "sd_ratio"):
            assert np.allclose(rows[cohort][field], rows64[cohort][field], rtol=0, atol=1e-9), (cohort, field)


@pytest.mark.parametrize("method", ["mean", "ssgsea"])
def test_pathway_consistency_reads_the_planted_design(method):
    (faithful, _), (decoupled, drows) = _device(method, "faithful"), _device(method, "decoupled")
    print(method, faithful["pwc_pearson_min"], faithful["pwc_rmse_max"], np.nanmax(np.abs(drows["synthetic"]["pearson"])),
          decoupled["pwc_rmse_mean"])
    assert faithful["pwc_pearson_min"] >= 0.98 and faithful["pwc_rmse_max"] <= 0.15
    assert np.nanmax(np.abs(drows["synthetic"]["pearson"])) <= 5 / np.sqrt(N_SYNTH) and decoupled["pwc_rmse_mean"] >= 1.0
    assert faithful["pwc_real_pearson_min"] >= 1 - 1e-9 and faithful["pwc_real_rmse_max"] <= 1e-6
    assert faithful["pwc_pathways"] == 7 and faithful["pwc_constant"] == 0 and faithful["pwc_rows_nonfinite"] == 0


def test_scorer_frames_device_frames_and_state():
    c = _cohorts("mean")
    genes = [f"G{i}" for i in range(N_GENES)]
    sets = {name: [genes[i] for i in members] for name, members in c["sets"].items()}
    sets["ABSENT"] = ["Q1", "Q2", "Q3", "Q4", "Q5"]
    host = PW.PathwayScorer(sets, genes, method="zscore", kernels=NumpyKernels()).fit(c["real"])
    for method in ("mean", "zscore", "ssgsea"):
        s = PW.PathwayScorer(sets, genes, method=method).fit(pd.DataFrame(c["real"], columns=genes))
        assert s.names == c["names"] and s.skipped == 1 and s.device.type == "cuda"
        frame = s.score(pd.DataFrame(c["synth"], columns=genes, index=[f"p{i}" for i in range(N_SYNTH)]), standardize=True)
        assert isinstance(frame, pd.DataFrame) and list(frame.columns) == c["names"] and frame.index[3] == "p3"
        dev = s.score(DeviceFrame(torch.from_numpy(c["synth"]).cuda(), genes), standardize=True)
        assert isinstance(dev, DeviceFrame) and list(dev.columns) == c["names"] and dev.values.dtype == torch.float64
        bare = s.score(torch.from_numpy(c["synth"]).cuda(), standardize=True)
        assert np.array_equal(frame.values, dev.values.cpu().numpy()) and torch.equal(bare, dev.values)
        back = PW.PathwayScorer.from_state(s.state())
        assert torch.equal(back.score(torch.from_numpy(c["synth"]).cuda(), standardize=True), bare)
        if method == "zscore":                                 # the device fit against the stand-in's: the centre within an fp32 ulp
            assert np.allclose(s.center, host.center, rtol=3e-7, atol=0) and np.allclose(s.scale, host.scale, rtol=3e-7, atol=0)
            assert np.allclose(s.mu, host.mu, rtol=0, atol=1e-5) and np.allclose(s.sd, host.sd, rtol=1e-5)
        if method == "mean":
            assert np.allclose(frame.values, c["z"], rtol=0, atol=1e-9)


def test_validate_all_carries_the_consistency_keys():
    c = _cohorts("mean")
    rs = np.random.default_rng(0)
    genes = [f"G{i}" for i in range(N_GENES)]

    def frames(expr, block, n):
        mut = pd.DataFrame((rs.random((n, 20)) < 0.3).astype(np.float32), columns=[f"M{i}" for i in range(20)])
        return mut, pd.DataFrame(expr, columns=genes), pd.DataFrame(block, columns=c["names"])

    pgm = pd.DataFrame(0, index=["ABSENT"] + genes[::-1], columns=c["names"])
    for name, members in c["sets"].items():
        pgm.loc[[genes[i] for i in members], name] = 1
    real, synth = frames(c["real"], c["real_block"], 600), frames(c["synth"], c["faithful"], N_SYNTH)
    val = BiologicalValidator(CONF)
    np.random.seed(5)
    plain = val.validate_all(*real, *synth, pathway_gene_matrix=pgm)
    np.random.seed(5)
    full = val.validate_all(*real, *synth, pathway_gene_matrix=pgm, consistency=True)
    assert not any(k.startswith("pwc_") for k in plain)
    extra = [k for k in full if k not in plain]
    assert extra and all(k.startswith("pwc_") for k in extra) and [k for k in full if k in plain] == list(plain)
    want = _device("mean", "faithful")[0]
    assert set(extra) == set(want) and all(full[k] == want[k] for k in ("pwc_pathways", "pwc_rmse_max_pathway"))
    assert abs(full["pwc_pearson_min"] - want["pwc_pearson_min"]) <= 1e-9 and full["pwc_real_rmse_max"] <= 1e-6
    ranked = val.validate_all(*real, *synth, pathway_gene_matrix=pgm, consistency=True, consistency_method="ssgsea")
    assert ranked["pwc_pathways"] == 7 and ranked["pwc_pearson_min"] < full["pwc_pearson_min"]   # a mean-made block under another method
    with pytest.raises(ValueError):
        val.validate_all(*real, *synth, consistency=True)
    sharded = BiologicalValidator(CONF, sharded=True)          # no process group: one shard, the same figures
    assert sharded.pathway_consistency(c["synth"], c["faithful"], c["sets"], c["real"], c["real_block"]) == want


def test_column_slices_of_the_combined_matrix_are_read_in_place():
    """The expression and pathway blocks as column slices of one [mutation | expression | pathway] device matrix reach the kernels as
    they are -- same address, row stride of the combined matrix -- and give the figures of separate contiguous copies."""
    c = _cohorts("ssgsea")
    n_mut, S = PAD, len(c["names"])
    combined = {}
    for name, expr, block in (("real", c["real"], c["real_block"]), ("synth", c["synth"], c["faithful"])):
        mut = np.zeros((expr.shape[0], n_mut), dtype=np.float32)
        combined[name] = torch.from_numpy(np.concatenate([mut, expr, block], axis=1)).cuda()
    e, p = slice(n_mut, n_mut + N_GENES), slice(n_mut + N_GENES, n_mut + N_GENES + S)
    scorer = PW.PathwayScorer(c["sets"], list(range(N_GENES)), method="ssgsea")
    view = combined["synth"][:, e]
    seen = scorer._matrix(view)
    assert seen.data_ptr() == view.data_ptr() == combined["synth"].data_ptr() + 4 * n_mut and seen.stride(0) == n_mut + N_GENES + S
    block = PW._block(combined["synth"][:, p], c["names"], scorer.device, N_SYNTH)
    assert block.data_ptr() == combined["synth"][:, p].data_ptr() and block.stride(0) == n_mut + N_GENES + S
    assert torch.equal(scorer.score(view), scorer.score(view.contiguous()))
    val = BiologicalValidator(CONF)
    sliced = val.pathway_consistency(combined["synth"][:, e], combined["synth"][:, p], c["sets"], combined["real"][:, e],
                                     combined["real"][:, p], method="ssgsea")
    assert sliced == _device("ssgsea", "faithful")[0]
