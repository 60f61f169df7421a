"""GPU: ``osd_val_marginals`` (csrc/marginal.hip: col_tiles<false>, the segmented sort, marg_stats, marg_finish), and
``BiologicalValidator.marginal_fidelity`` above it, against the float64 / int64 restatement of tests/marginal_helpers.py evaluated on
the same fp32 inputs.

Kernel shapes (n1, n2, D): (1, 1, 1), (1, 7, 5), (5, 3, 6), (64, 65, 33), (257, 130, 130) -- small, row tails, column counts off the
wavefront width; (130, 4099, 66) many synthetic partners per real value and (4099, 130, 5) the reverse; (4097, 8193, 3) a segment over
two SEG_CHUNKs; (100, 1000, 5142) the reference's width; (20001, 30011, 8) windows beyond the LDS stage of 4096 values (on a binary or a
signed-zero column a run that crosses from one value to the next asks for every equal value of the other cohort: 13 500 ones, 24 000
zeros; heavy ties with eight values, 3750 each, stay inside it).  Each runs dense, as an aligned and as
an unaligned column slice of a wider matrix full of 1000s, on eight kinds of data (marginal_helpers.KINDS; ``identical`` is the real
cohort in another row order, so there n2 = n1).

  * ks_dmax, ks_dmin, below, above EQUAL the int64 restatement, and the extremes equal osd_val_ks_extremes on the leading columns;
  * integer data: w1 is the correctly rounded quotient of the exact integer sum by n1 n2 -- the kernel's double sum is then exact --,
    so rint(w1 n1 n2) is that sum;
  * real data: |w1 - w1_ref| <= (n1 + n2 + 4) 2^-52 w1_ref: one rounding each for the difference, the product and the quotient, the
    rest a double sum of at most n1 + n2 non-negative terms in whatever order;
  * identical cohorts: every figure exactly 0; disjoint supports: dmax = n1 n2 or dmin = -n1 n2, and every synthetic value outside;
  * chunk_cols 0, 1, 7 and D and a repeated call: identical bits; bad arguments: OSD_EINVAL.

End to end (600 real, 900 synthetic, D = 130 in three blocks): the keys that derive from integers (KS, range shares, counts, argmax
indices) EQUAL the float64 pipeline -- the validator's own host code over the float64 kernels --, the W1-scaled keys are held to it.
    Measured, the largest |device - float64| / |float64| over the W1-scaled keys: faithful 7.224e-15, shifted 2.881e-15, collapsed
    2.804e-15, zero_lost 7.315e-15, outside 1.873e-15.  Asserted: 4 x the largest.  In the same run the per-feature W1 equalled the
    float64 restatement to the bit on four of the five samplers (zero_lost: one ulp, 2.2e-16) and the real columns' sample sd
    differed by up to 7.83e-15 -- the device's column moments, a double sum in another order, are the whole of it."""
import ctypes as C_
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import (BiologicalValidator, DeviceKernels, marginal_summary, real_sample_sd,
                                                         sharded_marginals)
from marginal_helpers import INTEGER_KINDS, KINDS, U52, NumpyKernels, make_case, marginals64

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 5), (5, 3, 6), (64, 65, 33), (257, 130, 130), (130, 4099, 66), (4099, 130, 5), (4097, 8193, 3), (100, 1000, 5142),
          (20001, 30011, 8)]
LAYOUTS = ["dense", "slice_aligned", "slice_unaligned"]
INT_FIELDS = ("ks_dmax", "ks_dmin", "below", "above")
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
def _case(kind, n1, n2, D):
    if kind == "identical":
        n2 = n1
    a, b = make_case(kind, n1, n2, D)
    return a, b, marginals64(a, b, integer=kind in INTEGER_KINDS)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n1,n2,D", SHAPES)
def test_marginals_against_restatement(n1, n2, D, kind, layout):
    a, b, ref = _case(kind, n1, n2, D)
    n2 = b.shape[0]
    k = _kernels()
    got = k.marginals(_layout(a, layout), _layout(b, layout))
    for name in INT_FIELDS:
        assert got[name].dtype == np.int64 and got[name].shape == (D,)
        assert np.array_equal(got[name], ref[name]), (name, int((got[name] != ref[name]).sum()), D)
    nf = min(D, 100)
    dmax, dmin = k.ks_extremes(_t(a), _t(b), nf)
    assert np.array_equal(got["ks_dmax"][:nf], dmax) and np.array_equal(got["ks_dmin"][:nf], dmin)
    w1, want = got["w1"], ref["w1"]
    assert w1.dtype == np.float64 and w1.shape == (D,) and np.isfinite(w1).all()
    if kind in INTEGER_KINDS:
        exact = ref["w1_int"]
        assert int(exact.max()) < 2 ** 52
        assert np.array_equal(w1, exact.astype(np.float64) / (float(n1) * float(n2)))
        assert np.array_equal(np.rint(w1 * n1 * n2).astype(np.int64), exact)
    err, bound = np.abs(w1 - want), (n1 + n2 + 4) * U52 * want
    print(f"marginals {n1}x{n2}x{D} {kind} {layout}: max w1 err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    if kind == "identical":
        assert not any(got[name].any() for name in INT_FIELDS) and not w1.any()
    if kind == "disjoint":
        assert (got["ks_dmax"][0::2] == n1 * n2).all() and (got["ks_dmin"][1::2] == -n1 * n2).all()
        assert (got["above"][0::2] == n2).all() and (got["below"][1::2] == n2).all()
    if kind == "constant_column":
        assert got["ks_dmax"][0] == 0 and got["ks_dmin"][0] == 0 and w1[0] == 0.0      # the same constant in both cohorts


@pytest.mark.parametrize("kind", ["normal", "zero_inflated"])
@pytest.mark.parametrize("n1,n2,D", SHAPES)
def test_marginals_same_bits_at_every_chunk(n1, n2, D, kind):
    a, b, _ = _case(kind, n1, n2, D)
    k, x, y = _kernels(), _t(a), _t(b)
    first = k.marginals(x, y)
    for chunk in (0, 1, 7, D):
        again = k.marginals(x, y, chunk_cols=chunk)
        for name in INT_FIELDS:
            assert np.array_equal(again[name], first[name]), (name, chunk)
        assert np.array_equal(again["w1"].view(np.int64), first["w1"].view(np.int64)), chunk
    timed = k.marginals(x, y, chunk_cols=7, phases=True)
    assert np.array_equal(timed["w1"].view(np.int64), first["w1"].view(np.int64)) and timed["phase_ms"].shape == (3,)
    assert (timed["phase_ms"] >= 0).all() and timed["phase_ms"].sum() > 0


def test_marginals_argument_errors():
    lib = L.lib()
    x = torch.zeros((8, 8), device="cuda")
    outs = [np.zeros(8, dtype=np.int64) for _ in range(5)]
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(real=x, n1=8, ld_real=8, synth=x, n2=8, ld_synth=8, D=8, chunk=0, drop=None):
        ptrs = [None if i == drop else C_.c_void_p(o.ctypes.data) for i, o in enumerate(outs)]
        return lib.osd_val_marginals(stream, 0, L.ptr(real), n1, ld_real, L.ptr(synth), n2, ld_synth, D, chunk, *ptrs)

    assert call() == L.OSD_OK and call(chunk=3) == L.OSD_OK and call(chunk=1000) == L.OSD_OK and call(D=4) == L.OSD_OK
    for bad in [dict(real=None), dict(synth=None), dict(n1=0), dict(n2=0), dict(n1=-1), dict(D=0), dict(D=-2), dict(ld_real=7), dict(ld_synth=7),
                dict(chunk=-1), dict(n1=1 << 27, n2=(1 << 26) + 1)] + [dict(drop=i) for i in range(5)]:
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error()
    k = _kernels()
    with pytest.raises(ValueError):
        k.marginals(x, x[:, :7])
    with pytest.raises(ValueError):
        k.marginals(x, x, chunk_cols=-1)


# ---- 2. marginal_fidelity end to end ----------------------------------------------------------------------------------------------
N_REAL, N_SYNTH = 600, 900
BLOCKS = {"mutations": 20, "expression": 90, "pathways": 20}
E2E_D = 130
SHIFTED, COLLAPSED, PUSHED_UP, PUSHED_DOWN = 115, 117, 112, 113        # pathway columns
E2E_OBSERVED = 7.315e-15         # measured max |device - float64| / |float64| over the W1-scaled keys of the five samplers
E2E_TOL = 4 * E2E_OBSERVED


@functools.lru_cache(maxsize=None)
def _params():
    rs = np.random.default_rng(28)
    return 0.05 + 0.4 * rs.random(20), 2.0 * rs.standard_normal(20), 0.5 + rs.random(20)      # mutation rates, pathway means and sds


def _draw(n, seed):
    rates, mu, sd = _params()
    rs = np.random.default_rng(seed)
    mut = (rs.random((n, 20)) < rates).astype(np.float64)
    expr = np.where(rs.random((n, 90)) < 0.3, 0.0, rs.gamma(2.0, 1.5, (n, 90)))            # zero-inflated, right-skewed
    pw = mu + sd * rs.standard_normal((n, 20))
    return np.concatenate([mut, expr, pw], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _cohorts():
    _, mu, sd = _params()
    real = _draw(N_REAL, 1)
    faithful = _draw(N_SYNTH, 2)
    shifted = _draw(N_SYNTH, 3)
    shifted[:, SHIFTED] += np.float32(sd[SHIFTED - 110])                                      # one standard deviation up
    collapsed = _draw(N_SYNTH, 4)
    collapsed[:, COLLAPSED] = (mu[COLLAPSED - 110] + 0.1 * (collapsed[:, COLLAPSED] - mu[COLLAPSED - 110])).astype(np.float32)
    zero_lost = _draw(N_SYNTH, 5)
    expr = zero_lost[:, 20:110]
    fill = np.random.default_rng(55).uniform(1e-6, 1e-3, expr.shape).astype(np.float32)
    expr[expr == 0] = fill[expr == 0]                                                         # a sampler that never says "not expressed"
    outside = _draw(N_SYNTH, 6)
    outside[:45, PUSHED_UP] = real[:, PUSHED_UP].max() + 1.0
    outside[:9, PUSHED_DOWN] = real[:, PUSHED_DOWN].min() - 1.0
    return real, {"faithful": faithful, "shifted": shifted, "collapsed": collapsed, "zero_lost": zero_lost, "outside": outside}


CASES = ["faithful", "shifted", "collapsed", "zero_lost", "outside"]


@functools.lru_cache(maxsize=None)
def _pipeline64(name):
    """The float64 pipeline: the validator's own host code over the float64 kernels."""
    from osteosarcoma_diffusionmodel_amd.validation import corr_block_bounds
    real, synth = _cohorts()
    x, y = torch.from_numpy(real), torch.from_numpy(synth[name])
    rows = sharded_marginals(ShardComm(False), NumpyKernels(), x, y)
    rows["real_sd"] = real_sample_sd(NumpyKernels(), x)
    bounds, names = corr_block_bounds(BLOCKS, E2E_D)
    return marginal_summary(rows, bounds, names), rows


@functools.lru_cache(maxsize=None)
def _device(name):
    real, synth = _cohorts()
    return BiologicalValidator(CONF).marginal_fidelity(real, synth[name], blocks=BLOCKS, return_rows=True)


def _compare(got, want, tol):
    """Keys in the same order; the W1-scaled ones within tol (relative), every other one -- a function of integers alone -- equal."""
    assert list(got) == list(want)
    worst = 0.0
    for key, w in want.items():
        g = got[key]
        if "w1_scaled" in key and not key.endswith("_feature"):
            worst = max(worst, abs(g - w) / abs(w) if w else abs(g))
            assert abs(g - w) <= tol * abs(w), (key, g, w)
        else:
            assert g == w, (key, g, w)
    return worst


@pytest.mark.parametrize("name", CASES)
def test_marginal_fidelity_equals_float64_pipeline(name):
    (got, rows), (want, rows64) = _device(name), _pipeline64(name)
    for field in INT_FIELDS:
        assert np.array_equal(rows[field], rows64[field]), field
    assert rows["n1"] == N_REAL and rows["n2"] == N_SYNTH and rows["ks"].shape == (E2E_D,) and rows["worst_ks"].shape == (10,)
    assert rows["worst_ks"][0] == got["marginal_ks_max_feature"] and (np.diff(rows["ks"][rows["worst_ks"]]) <= 0).all()
    assert got["marginal_features"] == E2E_D and got["marginal_constant_features"] == 0
    worst = _compare(got, want, E2E_TOL)
    w1_dev = float(np.max(np.abs(rows["w1"] - rows64["w1"]) / np.maximum(rows64["w1"], 1e-300)))
    sd_dev = float(np.max(np.abs(rows["real_sd"] - rows64["real_sd"]) / rows64["real_sd"]))
    print(f"marginal_fidelity {name}: largest |device - float64| / |float64| over the W1-scaled keys = {worst:.3e} "
          f"(per feature: w1 {w1_dev:.3e}, real sd {sd_dev:.3e})")


def test_marginal_fidelity_faithful():
    got = _device("faithful")[0]
    # two-sample KS noise at (600, 900): sqrt(-ln(alpha / 2) / 2) sqrt((n1 + n2) / (n1 n2)) at alpha = 1e-4 over 130 features
    assert got["marginal_ks_max"] < np.sqrt(-np.log(0.5e-4) / 2.0) * np.sqrt((N_REAL + N_SYNTH) / (N_REAL * N_SYNTH))
    assert got["marginal_w1_scaled_max"] < 0.25 and got["marginal_out_of_range_max"] < 0.02


def test_marginal_fidelity_shifted_feature():
    got, rows = _device("shifted")
    assert got["marginal_ks_max_feature"] == SHIFTED and got["marginal_w1_scaled_max_feature"] == SHIFTED
    # a shift by one sd: KS = 2 Phi(1/2) - 1 = 0.383 and W1 = 1 sd, up to sampling
    assert 0.3 < got["marginal_ks_max"] < 0.47 and 0.85 < got["marginal_w1_scaled_max"] < 1.15
    assert got["marginal_ks_max_pathways"] == got["marginal_ks_max"] > got["marginal_ks_max_expression"] + 0.15
    assert rows["worst_ks"][0] == SHIFTED


def test_marginal_fidelity_collapsed_feature():
    got, rows = _device("collapsed")
    assert got["marginal_ks_max_feature"] == COLLAPSED
    # sd x 0.1 about the mean: KS -> sup |Phi(z) - Phi(10 z)| = 0.40, W1 -> 0.9 E|z| = 0.72 sd
    assert 0.33 < rows["ks"][COLLAPSED] < 0.47 and 0.6 < rows["w1_scaled"][COLLAPSED] < 0.85
    assert rows["below"][COLLAPSED] == 0 and rows["above"][COLLAPSED] == 0


def test_marginal_fidelity_lost_zero_inflation():
    real, synth = _cohorts()
    got, rows = _device("zero_lost")
    share = (real[:, 20:110] == 0).mean(0)                    # the real columns' zero shares, 0.3 each up to sampling
    # at v = 0 the real CDF stands at the zero share and the synthetic one at 0; above 1e-3 the two agree up to sampling noise, far
    # below 0.3: a column's KS distance is its real zero share, plus at most the real values inside (0, 1e-3] (a 2e-7 chance each)
    assert (rows["ks"][20:110] >= share).all() and (rows["ks"][20:110] <= share + 2.0 / N_REAL).all()
    assert share.mean() <= got["marginal_ks_mean_expression"] <= share.mean() + 2.0 / N_REAL and abs(share.mean() - 0.3) < 0.01
    assert got["marginal_ks_mean_mutations"] < 0.05 and got["marginal_ks_mean_pathways"] < 0.06
    faithful = _device("faithful")[0]
    assert faithful["marginal_ks_mean_expression"] < 0.06
    assert got["marginal_w1_scaled_mean_expression"] < 0.1    # the mass moved by at most 1e-3: KS sees it, W1 does not


def test_marginal_fidelity_out_of_range_shares():
    real, synth = _cohorts()
    got, rows = _device("outside")
    y = synth["outside"]
    out = (y < real.min(0)) | (y > real.max(0))
    assert np.array_equal(rows["below"] + rows["above"], out.sum(0))
    assert got["marginal_out_of_range_share"] == int(out.sum()) / (float(N_SYNTH) * E2E_D)
    assert got["marginal_out_of_range_max"] == out.sum(0).max() / float(N_SYNTH) and out.sum(0).argmax() == PUSHED_UP
    assert rows["above"][PUSHED_UP] >= 45 and rows["below"][PUSHED_DOWN] >= 9
    assert got["marginal_out_of_range_max"] >= 45 / N_SYNTH


def test_marginal_fidelity_argument_errors():
    real, synth = _cohorts()
    val = BiologicalValidator(CONF)
    x, y = real, synth["faithful"]
    bad = np.array(x)
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match="real"):
        val.marginal_fidelity(bad, y)
    worse = np.array(y)
    worse[5, 100] = np.inf
    with pytest.raises(ValueError, match="synthetic"):
        val.marginal_fidelity(x, worse)
    with pytest.raises(ValueError, match="synthetic"):
        val.marginal_fidelity(x, y[:, :100])
    with pytest.raises(ValueError):
        val.marginal_fidelity(x, y, blocks={"a": 100, "b": 20})
    with pytest.raises(ValueError):
        val.marginal_fidelity(x[:0], y)


# ---- 3. row shards ----------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, q):
    import torch.distributed as dist
    from osteosarcoma_diffusionmodel_amd.parallel import shard_rows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        real, synth = _cohorts()
        off, cnt = shard_rows(N_SYNTH, rank, world)
        val = BiologicalValidator(CONF, sharded=True)
        assert val.comm.on
        res, rows = val.marginal_fidelity(real, synth["shifted"][off:off + cnt], blocks=BLOCKS, return_rows=True)
        q.put((rank, res, {name: rows[name] for name in INT_FIELDS + ("w1",)}))
    except Exception as e:
        q.put((rank, repr(e), None))
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_marginal_fidelity_equals_single_process():
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
    ref, ref_rows = _device("shifted")
    for _, r, rows in res:                                     # the kernel's bits do not depend on who calls it: everything is equal
        assert list(r) == list(ref) and all(r[key] == ref[key] for key in ref), (r, ref)
        assert all(np.array_equal(rows[name], ref_rows[name]) for name in INT_FIELDS)
        assert np.array_equal(rows["w1"].view(np.int64), ref_rows["w1"].view(np.int64))


# ---- 4. validate_all --------------------------------------------------------------------------------------------------------------
def test_validate_all_carries_the_marginal_keys():
    import pandas as pd
    real, synth = _cohorts()
    x, y = real, synth["shifted"]

    def frames(a):
        mut = pd.DataFrame(a[:, :20], columns=[f"M{i}" for i in range(20)])
        expr = pd.DataFrame(a[:, 20:110], columns=[f"G{i}" for i in range(90)])
        pw = pd.DataFrame(a[:, 110:], columns=[f"PW{i}" for i in range(20)])
        return mut, expr, pw

    val = BiologicalValidator(CONF)
    np.random.seed(5)
    plain = val.validate_all(*frames(x), *frames(y))
    np.random.seed(5)
    full = val.validate_all(*frames(x), *frames(y), marginals=True)
    assert not any(k.startswith("marginal_") for k in plain)
    extra = [k for k in full if k not in plain]
    assert all(k.startswith("marginal_") for k in extra) and [k for k in full if k in plain] == list(plain)
    assert all(full[k] == pytest.approx(plain[k], rel=1e-9, abs=1e-12, nan_ok=True) for k in plain)      # double atomics: last-bit freedom
    direct = _device("shifted")[0]
    assert extra == list(direct) and all(full[k] == direct[k] for k in extra)
    assert full["marginal_ks_max_feature"] == SHIFTED and f"{full['marginal_ks_max']:.4f}"
