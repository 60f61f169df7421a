"""CPU: the host side of ``BiologicalValidator.marginal_fidelity`` -- the float64 restatement of tests/marginal_helpers.py against
scipy, ``marginal_summary`` on hand-made rows, ``sharded_marginals`` over gloo with NumPy standing in for the device kernels, and
the C ABI / Python signatures."""
import inspect
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from marginal_helpers import INTEGER_KINDS, KINDS, NumpyKernels, coupling, ks_extremes64, make_case, marginals64

ROOT = Path(__file__).resolve().parent.parent


# ---- 1. the restatement against scipy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 7), (5, 3), (64, 65), (257, 130), (130, 1031), (600, 600)])
def test_coupling_weights(n1, n2):
    i, j, w = coupling(n1, n2)
    assert (w > 0).all() and int(w.sum()) == n1 * n2
    # the issue's closed form, pair by pair
    want = [(a, b, min((a + 1) * n2, (b + 1) * n1) - max(a * n2, b * n1)) for a in range(n1)
            for b in range(a * n2 // n1, ((a + 1) * n2 - 1) // n1 + 1)]
    assert [(int(a), int(b), int(c)) for a, b, c in zip(i, j, w)] == want
    longer, shorter = max(n1, n2), min(n1, n2)
    per_long = np.bincount(i if n1 >= n2 else j)
    assert per_long.max() <= -(-shorter // longer) + 1                    # at most ceil(shorter / longer) + 1 partners


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "identical"])
@pytest.mark.parametrize("n1,n2,D", [(1, 7, 5), (5, 3, 6), (64, 65, 9), (257, 130, 7), (130, 1031, 4)])
def test_restatement_equals_scipy(kind, n1, n2, D):
    from scipy import stats
    a, b = make_case(kind, n1, n2, D)
    r = marginals64(a, b, integer=kind in INTEGER_KINDS)
    for f in range(D):
        x, y = a[:, f].astype(np.float64), b[:, f].astype(np.float64)
        w = stats.wasserstein_distance(x, y)
        # scipy integrates |F_a - F_b| over the pooled range: each CDF value is a quotient rounded at magnitude <= 1, so ITS error is
        # absolute -- a few 2^-53 times the pooled range -- where the two CDFs nearly cancel (the restatement is exact on integers)
        spread = max(x.max(), y.max()) - min(x.min(), y.min())
        assert abs(r["w1"][f] - w) <= 16 * 2.0 ** -52 * max(w, spread), (f, r["w1"][f], w)
        ks = max(r["ks_dmax"][f], -r["ks_dmin"][f], 0) / (n1 * n2)
        assert ks == pytest.approx(stats.ks_2samp(x, y).statistic, rel=1e-13, abs=1e-15)
        assert r["below"][f] == (y < x.min()).sum() and r["above"][f] == (y > x.max()).sum()
    if kind in INTEGER_KINDS:
        assert np.array_equal(r["w1"], r["w1_int"].astype(np.float64) / (float(n1) * n2))
    if kind == "binary":                                                   # both distances reduce to |p - q|
        gap = np.abs(a.astype(np.float64).mean(0) - b.astype(np.float64).mean(0))
        assert np.allclose(r["w1"], gap, rtol=1e-12, atol=1e-15)
        assert np.allclose(np.maximum(r["ks_dmax"], -r["ks_dmin"]) / (n1 * n2), gap, rtol=1e-12, atol=1e-15)


def test_restatement_identical_and_disjoint():
    a, b = make_case("identical", 130, 130, 6)
    r = marginals64(a, b)
    assert not any(r[k].any() for k in ("ks_dmax", "ks_dmin", "w1", "below", "above"))
    a, b = make_case("disjoint", 64, 65, 4)
    r = marginals64(a, b)
    assert r["ks_dmax"][0::2].tolist() == [64 * 65] * 2 and r["ks_dmin"][1::2].tolist() == [-64 * 65] * 2
    assert r["above"][0::2].tolist() == [65] * 2 and r["below"][1::2].tolist() == [65] * 2
    assert ks_extremes64(np.array([0.0, 1.0]), np.array([2.0])) == (2, 0)


# ---- 2. marginal_summary on hand-made rows ----------------------------------------------------------------------------------------
def _rows(n1, n2, dmax, dmin, w1, below, above, sd):
    return {"n1": n1, "n2": n2, "ks_dmax": np.array(dmax, dtype=np.int64), "ks_dmin": np.array(dmin, dtype=np.int64),
            "w1": np.array(w1, dtype=np.float64), "below": np.array(below, dtype=np.int64), "above": np.array(above, dtype=np.int64),
            "real_sd": np.array(sd, dtype=np.float64)}


def test_summary_identical_cohorts_is_all_zero():
    from osteosarcoma_diffusionmodel_amd.validation import marginal_summary
    z = [0] * 6
    out = marginal_summary(_rows(10, 20, z, z, [0.0] * 6, z, z, [1.0, 2.0, 0.5, 1.0, 1.0, 3.0]), [0, 2, 6], ["a", "b"])
    assert out.pop("marginal_features") == 6
    assert list(out) == ["marginal_constant_features", "marginal_ks_mean", "marginal_ks_median", "marginal_ks_p95", "marginal_ks_max",
                         "marginal_ks_max_feature", "marginal_w1_scaled_mean", "marginal_w1_scaled_median", "marginal_w1_scaled_p95",
                         "marginal_w1_scaled_max", "marginal_w1_scaled_max_feature", "marginal_out_of_range_share",
                         "marginal_out_of_range_max", "marginal_ks_mean_a", "marginal_ks_max_a", "marginal_w1_scaled_mean_a",
                         "marginal_ks_mean_b", "marginal_ks_max_b", "marginal_w1_scaled_mean_b"]
    assert all(v == 0 for v in out.values())
    assert all(isinstance(v, (int, float)) and f"{v:.4f}" for v in out.values())       # validate_all logs each with :.4f


def test_summary_figures():
    from osteosarcoma_diffusionmodel_amd.validation import marginal_summary
    n1, n2 = 10, 20                                           # n1 n2 = 200
    rows = _rows(n1, n2, dmax=[20, 0, 100, 4, 0], dmin=[-10, -60, 0, -2, 0], w1=[0.5, 3.0, 0.25, 9.0, 0.0],
                 below=[0, 2, 0, 0, 5], above=[1, 0, 0, 0, 5], sd=[1.0, 2.0, 0.0, 0.5, 4.0])
    ks = np.array([0.1, 0.3, 0.5, 0.02, 0.0])
    scaled = np.array([0.5, 1.5, 18.0, 0.0])                  # feature 2 is constant: left out
    out = marginal_summary(rows, [0, 2, 3, 5], ["mut", "const", "expr"])
    assert out["marginal_features"] == 5 and out["marginal_constant_features"] == 1
    assert out["marginal_ks_mean"] == pytest.approx(ks.mean()) and out["marginal_ks_median"] == pytest.approx(0.1)
    assert out["marginal_ks_p95"] == pytest.approx(np.quantile(ks, 0.95)) and out["marginal_ks_max"] == 0.5
    assert out["marginal_ks_max_feature"] == 2                # the constant feature keeps its KS distance
    assert out["marginal_w1_scaled_mean"] == pytest.approx(scaled.mean()) and out["marginal_w1_scaled_median"] == pytest.approx(1.0)
    assert out["marginal_w1_scaled_p95"] == pytest.approx(np.quantile(scaled, 0.95)) and out["marginal_w1_scaled_max"] == 18.0
    assert out["marginal_w1_scaled_max_feature"] == 3         # an index into ALL columns, not into the non-constant ones
    assert out["marginal_out_of_range_share"] == pytest.approx(13 / 100) and out["marginal_out_of_range_max"] == pytest.approx(0.5)
    assert out["marginal_ks_mean_mut"] == pytest.approx(0.2) and out["marginal_ks_max_mut"] == pytest.approx(0.3)
    assert out["marginal_w1_scaled_mean_mut"] == pytest.approx(1.0)
    assert out["marginal_ks_mean_const"] == 0.5 and np.isnan(out["marginal_w1_scaled_mean_const"])
    assert out["marginal_ks_mean_expr"] == pytest.approx(0.01) and out["marginal_w1_scaled_mean_expr"] == pytest.approx(9.0)
    one = marginal_summary(rows, [0, 5], ["all"])             # one block: the global figures say it all
    assert not any(k.endswith("_all") for k in one) and one["marginal_ks_max"] == 0.5
    every = marginal_summary(_rows(n1, n2, [20], [0], [1.0], [0], [0], [0.0]), [0, 1], ["all"])     # nothing but a constant feature
    assert every["marginal_constant_features"] == 1 and np.isnan(every["marginal_w1_scaled_mean"])
    assert every["marginal_w1_scaled_max_feature"] == -1 and every["marginal_ks_max"] == 0.1
    for bad in ([0, 2, 6], [1, 5], [0, 3, 3, 5]):
        with pytest.raises(ValueError):
            marginal_summary(rows, bad, ["x"] * (len(bad) - 1))
    with pytest.raises(ValueError):
        marginal_summary(rows, [0, 2, 5], ["only one"])


def test_real_sample_sd():
    from osteosarcoma_diffusionmodel_amd.validation import real_sample_sd
    rs = np.random.default_rng(3)
    x = (rs.standard_normal((57, 9)) * 3.0 + 100.0).astype(np.float32)
    x[:, 4] = 7.25
    sd = real_sample_sd(NumpyKernels(), torch.from_numpy(x))
    assert sd[4] == 0.0 and np.allclose(sd, x.astype(np.float64).std(0, ddof=1), rtol=1e-12)
    assert not real_sample_sd(NumpyKernels(), torch.from_numpy(x[:1])).any()


# ---- 3. sharded_marginals over gloo -----------------------------------------------------------------------------------------------
def _shard_data():
    a, b = make_case("zero_inflated", 60, 101, 23, seed=4)    # 101 rows: ragged shards; 23 columns: ragged feature splits
    a[:, 5], b[:, 5] = np.round(a[:, 5]), np.round(b[:, 5])
    return torch.from_numpy(a), torch.from_numpy(b)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from osteosarcoma_diffusionmodel_amd.parallel import ShardComm, shard_rows
        from osteosarcoma_diffusionmodel_amd.validation import MARGINAL_FIELDS, sharded_marginals
        real, synth = _shard_data()
        off, cnt = shard_rows(synth.shape[0], rank, world)
        local = synth[off:off + cnt].contiguous()
        comm, k = ShardComm(True), NumpyKernels()
        assert comm.on and comm.world == world
        ref = sharded_marginals(ShardComm(False), k, real, synth)
        ok = True
        for gather_cols in (0, 1, 7, 23):
            got = sharded_marginals(comm, k, real, local, gather_cols=gather_cols)
            ok &= got["n1"] == 60 and got["n2"] == 101 and list(got) == list(ref)
            ok &= all(got[name].dtype == ref[name].dtype and np.array_equal(got[name], ref[name]) for name in MARGINAL_FIELDS)
        q.put((rank, bool(ok)))
    except Exception as e:                           # report instead of leaving the parent to time out
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_marginals_equal_single_process_gloo(world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(r, True) for r in range(world)]


# ---- 4. the C ABI and the Python signatures ---------------------------------------------------------------------------------------
def test_header_and_ctypes_entries():
    from osteosarcoma_diffusionmodel_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "osdiff.h").read_text(), flags=re.S)
    for name in ("osd_val_marginals", "osd_val_marginals_timed", "osd_val_marginals_auto_chunk"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in L.exported_symbols() and hasattr(L.lib(), name)
    decl = re.search(r"int osd_val_marginals\s*\((.*?)\);", text, flags=re.S).group(1)
    assert [p.split()[-1].lstrip("*") for p in decl.split(",")] == ["stream", "device", "real", "n1", "ld_real", "synth", "n2", "ld_synth",
                                                                    "D", "chunk_cols", "ks_dmax", "ks_dmin", "w1", "below", "above"]
    assert len(L._SIGNATURES["osd_val_marginals"][1]) == 15


def test_argument_errors_without_gpu():
    """The argument check comes before anything touches a device."""
    import ctypes as C
    from osteosarcoma_diffusionmodel_amd import _lib as L
    lib = L.lib()
    out = [(C.c_int64 * 4)() for _ in range(5)]
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(real=p, n1=4, ld_real=4, synth=p, n2=4, ld_synth=4, D=4, chunk=0, outs=out):
        return lib.osd_val_marginals(None, 0, real, n1, ld_real, synth, n2, ld_synth, D, chunk, *[C.cast(o, C.c_void_p) if o is not None else None
                                                                                                  for o in outs])

    bads = [dict(real=None), dict(synth=None), dict(n1=0), dict(n2=0), dict(n2=-3), dict(D=0), dict(ld_real=3), dict(ld_synth=3), dict(chunk=-1),
            dict(n1=1 << 27, n2=(1 << 26) + 1)] + [dict(outs=[None if i == j else o for j, o in enumerate(out)]) for i in range(5)]
    for bad in bads:
        assert call(**bad) == L.OSD_EINVAL, bad
        assert L.last_error()
    assert lib.osd_val_marginals_auto_chunk(125000, 125000, 2000) == 128          # 256 MiB / (8 x 250 000) = 134, in whole tiles of 64
    assert lib.osd_val_marginals_auto_chunk(1000000, 1000000, 2000) == (256 << 20) // (8 * 2000000) == 16
    assert lib.osd_val_marginals_auto_chunk(100, 3000, 5142) == 5142 and lib.osd_val_marginals_auto_chunk(1 << 30, 1 << 20, 7) == 1
    assert lib.osd_val_marginals_auto_chunk(0, 5, 5) == L.OSD_EINVAL


def test_python_signatures():
    from osteosarcoma_diffusionmodel_amd import validation as V
    sig = inspect.signature(V.BiologicalValidator.marginal_fidelity)
    assert list(sig.parameters)[:5] == ["self", "real", "synthetic", "blocks", "return_rows"]
    assert sig.parameters["blocks"].default is None and sig.parameters["return_rows"].default is False
    assert inspect.signature(V.BiologicalValidator.validate_all).parameters["marginals"].default is False
    assert list(inspect.signature(V.DeviceKernels.marginals).parameters)[:4] == ["self", "real", "synth", "chunk_cols"]
    assert inspect.signature(V.DeviceKernels.marginals).parameters["chunk_cols"].default == 0
    assert list(inspect.signature(V.sharded_marginals).parameters)[:4] == ["comm", "k", "real", "synth_local"]
    assert list(inspect.signature(V.marginal_summary).parameters) == ["rows", "bounds", "names"]
    assert "p-value" in V.BiologicalValidator.marginal_fidelity.__doc__ and "marginal_fidelity" in V.BiologicalValidator.statistical_tests.__doc__
