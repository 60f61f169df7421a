"""CPU: the host side of the correlation-structure metrics (osteosarcoma_diffusionmodel_amd/validation.py) -- ``frechet_distance`` on
cases with a closed form, ``corr_summary`` on hand-built sums and against the definitions (tests/corr_helpers.py),
``sharded_centered_gram`` over gloo with a numpy stand-in for the device kernels, and the argument errors of
``BiologicalValidator.correlation_fidelity`` that are raised before any device call (the GPU tests run the kernels)."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import validation as V
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm, shard_rows
from osteosarcoma_diffusionmodel_amd.validation import (BiologicalValidator, corr_block_bounds, corr_summary, frechet_distance,
                                                        sharded_centered_gram)
from corr_helpers import (FRECHET_KEYS, SUMMARY_KEYS, NumpyKernels, cohorts, compare_stats, frechet_oracle, gram64, summary_oracle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_rows_constant_mirrors_the_header():
    text = open(os.path.join(ROOT, "include", "osdiff.h")).read()
    import re
    assert int(re.search(r"#define\s+OSD_COV_SLAB_ROWS\s+(\d+)", text).group(1)) == V.COV_SLAB_ROWS
    assert int(re.search(r"#define\s+OSD_CORR_STATS\s+(\d+)", text).group(1)) == L.OSD_CORR_STATS == 7
    assert V.COV_SLAB_ROWS % 32 == 0


# ---- frechet_distance -----------------------------------------------------------------------------------------------------------
def _spd(rs, D, rank=None):
    a = rs.standard_normal((rank or 2 * D, D))
    return a.T @ a / a.shape[0]


def test_frechet_identical_inputs_give_zero():
    rs = np.random.default_rng(0)
    S, mu = _spd(rs, 12), rs.standard_normal(12)
    out = frechet_distance(mu, S, mu, S)
    assert list(out) == FRECHET_KEYS and all(type(v) is float for v in out.values())
    assert out["frechet_mean_term"] == 0.0 and 0.0 <= out["frechet_distance"] <= 1e-9 * np.trace(S)


def test_frechet_diagonal_covariances():
    s1, s2 = np.array([1.0, 2.0, 3.0]), np.array([2.0, 1.0, 0.5])
    mu1, mu2 = np.zeros(3), np.ones(3)
    out = frechet_distance(mu1, np.diag(s1 ** 2), mu2, np.diag(s2 ** 2))
    assert out["frechet_distance"] == pytest.approx(11.25, rel=1e-12)        # sum (sigma1 - sigma2)^2 + |dmu|^2 = (1 + 1 + 6.25) + 3
    assert out["frechet_mean_term"] == pytest.approx(3.0, rel=1e-15) and out["frechet_cov_term"] == pytest.approx(8.25, rel=1e-12)


def test_frechet_commuting_covariances():
    rs = np.random.default_rng(1)
    q, _ = np.linalg.qr(rs.standard_normal((7, 7)))                          # a shared, non-trivial eigenbasis
    l1, l2 = rs.uniform(0.1, 4.0, 7), rs.uniform(0.1, 4.0, 7)
    S1, S2 = (q * l1) @ q.T, (q * l2) @ q.T
    assert np.abs(S1 - np.diag(np.diag(S1))).max() > 0.05                    # not diagonal
    mu1, mu2 = rs.standard_normal(7), rs.standard_normal(7)
    want = ((mu1 - mu2) ** 2).sum() + ((np.sqrt(l1) - np.sqrt(l2)) ** 2).sum()
    assert frechet_distance(mu1, S1, mu2, S2)["frechet_distance"] == pytest.approx(want, rel=1e-10)


def test_frechet_general_case_against_the_product_eigenvalues():
    rs = np.random.default_rng(2)
    S1, S2 = _spd(rs, 9), _spd(rs, 9) * 1.7
    mu1, mu2 = rs.standard_normal(9), rs.standard_normal(9)
    got = frechet_distance(mu1, S1, mu2, S2)
    assert got["frechet_distance"] == pytest.approx(frechet_oracle(mu1, S1, mu2, S2), rel=1e-9)
    assert got["frechet_distance"] == pytest.approx(got["frechet_mean_term"] + got["frechet_cov_term"], rel=1e-15)


def test_frechet_one_feature():
    out = frechet_distance([1.0], [[4.0]], [3.0], [[9.0]])                   # (1 - 3)^2 + (2 - 3)^2
    assert out["frechet_distance"] == pytest.approx(5.0, rel=1e-12)
    assert frechet_distance(2.0, 4.0, 2.0, 4.0)["frechet_distance"] == pytest.approx(0.0, abs=1e-12)


def test_frechet_rank_deficient_and_symmetric():
    rs = np.random.default_rng(3)
    x, y = rs.standard_normal((50, 80)), rs.standard_normal((50, 80)) * 1.3 + 0.2      # 50 rows, 80 features: rank <= 49
    mu1, G1 = gram64(x)
    mu2, G2 = gram64(y)
    S1, S2 = G1 / 49, G2 / 49
    assert np.linalg.matrix_rank(S1) < 80
    a, b = frechet_distance(mu1, S1, mu2, S2), frechet_distance(mu2, S2, mu1, S1)
    for out in (a, b):
        assert all(math.isfinite(v) and v >= 0.0 for v in out.values())
    assert a["frechet_distance"] == pytest.approx(b["frechet_distance"], rel=1e-9)
    assert a["frechet_distance"] == pytest.approx(frechet_oracle(mu1, S1, mu2, S2), rel=1e-6)      # eigvals of a singular product
    same = frechet_distance(mu1, S1, mu1, S1)
    assert 0.0 <= same["frechet_distance"] <= 1e-9 * np.trace(S1)
    with pytest.raises(ValueError):
        frechet_distance(mu1, S1, mu2[:-1], S2)
    with pytest.raises(ValueError):
        frechet_distance(mu1, S1 * np.nan, mu2, S2)


# ---- corr_summary ---------------------------------------------------------------------------------------------------------------
def test_corr_summary_hand_built():
    # two blocks, pairs (0,0), (0,1), (1,1)
    stats = {"constant_columns": 1, "pairs": np.array([3, 4, 1]), "sum_abs": np.array([0.3, 0.8, 0.05]),
             "sum_sq": np.array([0.05, 0.2, 0.0025]), "max_abs": np.array([0.2, 0.4, 0.05]), "strong_pairs": np.array([2, 1, 0]),
             "strong_agree": np.array([2, 0, 0]), "strong_sum_abs": np.array([0.25, 0.4, 0.0])}
    s = corr_summary(stats, [0, 3, 5], ["mut", "expr"])
    assert list(s) == SUMMARY_KEYS + ["corr_mean_abs_diff_mut_mut", "corr_mean_abs_diff_mut_expr", "corr_mean_abs_diff_expr_expr"]
    assert s["corr_pairs"] == 8 and s["corr_constant_columns"] == 1 and s["corr_strong_pairs"] == 3
    assert s["corr_mean_abs_diff"] == pytest.approx(1.15 / 8) and s["corr_rms_diff"] == pytest.approx(math.sqrt(0.2525 / 8))
    assert s["corr_max_abs_diff"] == 0.4 and s["corr_frobenius_diff"] == pytest.approx(math.sqrt(0.505))
    assert s["corr_strong_sign_agreement"] == pytest.approx(2 / 3) and s["corr_strong_mean_abs_diff"] == pytest.approx(0.65 / 3)
    assert s["corr_mean_abs_diff_mut_mut"] == pytest.approx(0.1) and s["corr_mean_abs_diff_mut_expr"] == pytest.approx(0.2)
    assert s["corr_mean_abs_diff_expr_expr"] == pytest.approx(0.05)
    for k, v in s.items():
        assert type(v) is (int if k in ("corr_pairs", "corr_constant_columns", "corr_strong_pairs") else float), k
        f"{v:.4f}"                                                             # what validate_all's summary loop does
    one = corr_summary({k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in stats.items()}, [0, 3], ["all"])
    assert list(one) == SUMMARY_KEYS                                           # one block: no per-block keys
    with pytest.raises(ValueError):
        corr_summary(stats, [0, 3, 5], ["only"])
    with pytest.raises(ValueError):
        corr_summary(stats, [0, 2, 3, 5], ["a", "b", "c"])


def test_corr_summary_against_the_definitions():
    x, y = cohorts(120, 90, 23)
    x, y = x.copy(), y.copy()
    x[:, 4] = 2.0                                                              # a constant column (real cohort only)
    bounds, names = corr_block_bounds({"mutations": 5, "none": 0, "expression": 11, "pathways": 7}, 23)
    assert bounds == [0, 5, 16, 23] and names == ["mutations", "expression", "pathways"]
    (_, Gx), (_, Gy) = gram64(x), gram64(y)
    Gx[4, :] = Gx[:, 4] = 0.0
    for strong in (0.3, 5.0):
        stats = compare_stats(Gx, Gy, bounds, strong)
        got, ref = corr_summary(stats, bounds, names), summary_oracle(stats, names)
        assert list(got) == list(ref) and len(got) == len(SUMMARY_KEYS) + 6
        for k in ref:
            assert got[k] == pytest.approx(ref[k], rel=1e-14, nan_ok=True), k
        assert got["corr_constant_columns"] == 1 and got["corr_pairs"] == 22 * 21 // 2
        if strong > 1:                                                         # no pair is that strong: NaN, not a division error
            assert got["corr_strong_pairs"] == 0 and math.isnan(got["corr_strong_sign_agreement"])
            assert math.isnan(got["corr_strong_mean_abs_diff"])
        else:
            assert got["corr_strong_pairs"] > 10 and 0.0 < got["corr_strong_sign_agreement"] <= 1.0
    # against the plain definition over the 22 live columns
    keep = [c for c in range(23) if c != 4]
    d = (np.corrcoef(y[:, keep].astype(np.float64), rowvar=False) - np.corrcoef(x[:, keep].astype(np.float64), rowvar=False))[np.triu_indices(22, 1)]
    got = corr_summary(compare_stats(Gx, Gy, bounds, 0.3), bounds, names)
    assert got["corr_mean_abs_diff"] == pytest.approx(np.abs(d).mean(), rel=1e-9)
    assert got["corr_max_abs_diff"] == pytest.approx(np.abs(d).max(), rel=1e-9)
    assert got["corr_frobenius_diff"] == pytest.approx(np.sqrt(2 * (d * d).sum()), rel=1e-9)
    with pytest.raises(ValueError):
        corr_block_bounds({"a": 5, "b": 5}, 23)


def test_flat_stats_layout():
    flat = np.concatenate([[2.0], np.arange(14, dtype=np.float64)])
    st = V.corr_stats_from_flat(flat)
    assert st["constant_columns"] == 2 and st["pairs"].tolist() == [0, 7] and st["pairs"].dtype == np.int64
    assert st["sum_abs"].tolist() == [1.0, 8.0] and st["sum_sq"].tolist() == [2.0, 9.0] and st["max_abs"].tolist() == [3.0, 10.0]
    assert st["strong_pairs"].tolist() == [4, 11] and st["strong_agree"].tolist() == [5, 12] and st["strong_sum_abs"].tolist() == [6.0, 13.0]


# ---- sharded_centered_gram over gloo --------------------------------------------------------------------------------------------
def _shard_data():
    rs = np.random.RandomState(11)
    x = rs.randn(101, 9).astype(np.float32)                                    # 101 rows: ragged shards at world 2 and 3
    x[:, 2] += 0.8 * x[:, 1]
    x[:, 5] = (100.0 + rs.randn(101)).astype(np.float32)                       # mean 100, sd 1
    x[:, 7] = (1.0e5 + rs.randn(101)).astype(np.float32)                       # mean 1e5: n (mu - c)^2 is ~1e-5 of G_ii here
    return torch.from_numpy(x)


def _gram_close(G, ref, rel):
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref)))
    return bool((np.abs(G - ref) <= rel * scale).all())


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        x = _shard_data()
        sizes = {2: [70, 31], 3: [50, 0, 51]}[world]                           # uneven, and an empty shard
        off = sum(sizes[:rank])
        local = x[off:off + sizes[rank]].contiguous()
        mu_ref, ref = gram64(x.numpy())
        comm = ShardComm(True)
        ok = comm.on and comm.world == world
        n, mu, G = sharded_centered_gram(comm, NumpyKernels(), local)
        ok &= n == 101 and G.dtype == torch.float64 and tuple(G.shape) == (9, 9)
        ok &= bool(np.allclose(mu, mu_ref, rtol=1e-13, atol=0))
        ok &= _gram_close(G.numpy(), ref, 1e-9) and bool((G.numpy() == G.numpy().T).all())
        q.put((rank, bool(ok)))
    except Exception as e:                           # report instead of leaving the parent to time out
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_centered_gram_gloo(world):
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


def test_unsharded_gram_and_the_centre_correction():
    x = _shard_data()
    mu_ref, ref = gram64(x.numpy())
    n, mu, G = sharded_centered_gram(ShardComm(False), NumpyKernels(), x)
    assert n == 101 and np.allclose(mu, mu_ref, rtol=1e-13, atol=0)
    assert _gram_close(G.numpy(), ref, 1e-9)
    # what the kernel returns before the correction is NOT that close: the centre it sees is mu rounded to fp32
    raw = NumpyKernels.centered_gram(x, mu.astype(np.float32)).numpy()
    assert not _gram_close(raw, ref, 1e-9) and _gram_close(raw, ref, 1e-3)
    shard = shard_rows(101, 1, 3)
    assert shard == (34, 34)


# ---- argument errors that need no device ----------------------------------------------------------------------------------------
def test_correlation_fidelity_argument_errors_need_no_device():
    val = BiologicalValidator({"evaluation": {}}, device="cuda:0")
    x = np.zeros((9, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="same features"):
        val.correlation_fidelity(x, x[:, :3])
    with pytest.raises(ValueError, match="same features"):
        val.correlation_fidelity(x, np.zeros(9, dtype=np.float32))
    with pytest.raises(ValueError, match="at least 2"):
        val.correlation_fidelity(x[:1], x)
    with pytest.raises(ValueError, match="at least 2"):
        val.correlation_fidelity(x, x[:1])
    with pytest.raises(ValueError, match="add up"):
        val.correlation_fidelity(x, x, blocks={"a": 1, "b": 2})
    with pytest.raises(ValueError, match="strong"):
        val.correlation_fidelity(x, x, strong=float("nan"))
