"""CPU: the host side of the privacy audit (osteosarcoma_diffusionmodel_amd/validation.py) -- ``privacy_summary`` on
hand-written arrays with hand-computed results, and ``sharded_nearest_records`` over gloo with a numpy stand-in for the device
kernel (the GPU tests run the same functions on the real one)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from osteosarcoma_diffusionmodel_amd.parallel import shard_rows
from osteosarcoma_diffusionmodel_amd.validation import privacy_summary, sharded_nearest_records


def test_privacy_summary_hand_computed():
    rows = {
        "dcr": np.array([0.0, 1.0, 2.0, 0.0, 3.0]),
        "match": np.array([0, 2, 1, 1, 0]),
        "second": np.array([0.0, 2.0, np.inf, 4.0, 4.0]),       # 0/0, an infinite second neighbour
        "real_nn": np.array([2.5, 1.0, 1.5]),
        "dcr_holdout": np.array([0.0, 2.0, 1.0, 1.0, 3.0]),     # ties at rows 0 and 4
    }
    s = privacy_summary(rows)
    assert list(s) == ["privacy_dcr_min", "privacy_dcr_p05", "privacy_dcr_median", "privacy_exact_copy_fraction", "privacy_nndr_p05",
                       "privacy_nndr_median", "privacy_real_nn_median", "privacy_closer_than_real_nn_fraction",
                       "privacy_holdout_dcr_median", "privacy_closer_to_train_fraction"]
    assert all(type(v) is float for v in s.values())
    # dcr sorted: 0 0 1 2 3; the 5 % point sits at position 0.2 between the two zeros
    assert s["privacy_dcr_min"] == 0.0 and s["privacy_dcr_p05"] == 0.0 and s["privacy_dcr_median"] == 1.0
    assert s["privacy_exact_copy_fraction"] == 0.4
    # nndr = [0/0 -> 0, 0.5, 2/inf -> 0, 0, 0.75], sorted 0 0 0 0.5 0.75
    assert s["privacy_nndr_p05"] == 0.0 and s["privacy_nndr_median"] == 0.0
    assert s["privacy_real_nn_median"] == 1.5
    # real_nn[match] = [2.5, 1.5, 1.0, 1.0, 2.5]: dcr is smaller at rows 0, 1, 3
    assert s["privacy_closer_than_real_nn_fraction"] == 0.6
    assert s["privacy_holdout_dcr_median"] == 1.0
    # dcr < holdout at rows 1 and 3, equal at rows 0 and 4: (2 + 2 * 0.5) / 5
    assert s["privacy_closer_to_train_fraction"] == 0.6


def test_privacy_summary_without_holdout_and_quantiles():
    dcr = np.arange(1.0, 22.0)                               # 1 .. 21: the 5 % point is position 1.0 -> 2.0
    rows = {"dcr": dcr, "match": np.zeros(21, dtype=np.int64), "second": 2.0 * dcr, "real_nn": np.array([10.5, 3.0])}
    s = privacy_summary(rows)
    assert "privacy_holdout_dcr_median" not in s and "privacy_closer_to_train_fraction" not in s and len(s) == 8
    assert s["privacy_dcr_min"] == 1.0 and s["privacy_dcr_p05"] == 2.0 and s["privacy_dcr_median"] == 11.0
    assert s["privacy_exact_copy_fraction"] == 0.0
    assert s["privacy_nndr_p05"] == 0.5 and s["privacy_nndr_median"] == 0.5
    assert s["privacy_real_nn_median"] == 6.75
    assert s["privacy_closer_than_real_nn_fraction"] == 10 / 21      # dcr 1 .. 10 lie below real_nn[0] = 10.5
    with pytest.raises(ValueError):
        privacy_summary({"dcr": np.zeros(0), "match": np.zeros(0, dtype=np.int64), "second": np.zeros(0), "real_nn": np.ones(2)})


# ---- row-sharded nearest records over gloo, numpy standing in for the device kernel (the pattern of tests/test_parallel_cpu.py) ----
class NumpyKernels:
    """``nearest`` with the semantics of validation.DeviceKernels.nearest, float64 brute force."""

    @staticmethod
    def nearest(q, r, exclude=None):
        a, b = q.double().numpy(), r.double().numpy()
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        if exclude is not None:
            ex = exclude.numpy().astype(np.int64)
            ok = (ex >= 0) & (ex < b.shape[0])
            d2[np.nonzero(ok)[0], ex[ok]] = np.inf
        idx = d2.argmin(1)
        best = d2[np.arange(a.shape[0]), idx]
        idx = np.where(np.isinf(best), -1, idx)
        return torch.from_numpy(best.astype(np.float32)), torch.from_numpy(idx.astype(np.int32))


def _data():
    rs = np.random.RandomState(7)
    train = rs.randn(37, 12).astype(np.float32)             # 37 train, 101 synthetic rows: ragged shards at world 2 and 3
    holdout = rs.randn(20, 12).astype(np.float32)
    synth = rs.randn(101, 12).astype(np.float32)
    synth[:3] = train[[5, 30, 5]]                            # exact copies, two of the same record
    synth[3:9] = train[10:16] + 0.05 * rs.randn(6, 12).astype(np.float32)
    synth[9] = holdout[4]
    return torch.from_numpy(train), torch.from_numpy(synth), torch.from_numpy(holdout)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
        train, synth, holdout = _data()
        off, cnt = shard_rows(synth.shape[0], rank, world)
        local = synth[off:off + cnt].contiguous()
        k = NumpyKernels()
        whole = sharded_nearest_records(ShardComm(False), k, train, synth, holdout)
        comm = ShardComm(True)
        assert comm.on and comm.world == world
        got = sharded_nearest_records(comm, k, train, local, holdout)
        ok = list(got) == list(whole) == ["dcr", "match", "second", "real_nn", "dcr_holdout"]
        for key in whole:
            ok &= got[key].dtype == whole[key].dtype and np.array_equal(got[key], whole[key])
        ok &= got["dcr"].shape == (101,) and got["real_nn"].shape == (37,) and got["match"].dtype == np.int64
        ok &= got["match"][:3].tolist() == [5, 30, 5] and (got["dcr"][:3] == 0).all() and got["dcr_holdout"][9] == 0
        ok &= bool((got["second"] >= got["dcr"]).all()) and bool((got["real_nn"] > 0).all())
        no_holdout = sharded_nearest_records(comm, k, train, local)
        ok &= list(no_holdout) == ["dcr", "match", "second", "real_nn"] and np.array_equal(no_holdout["dcr"], whole["dcr"])
        ok &= privacy_summary(got) == privacy_summary(whole)
        q.put((rank, bool(ok)))
    except Exception as e:                           # report instead of leaving the parent to time out
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_nearest_records_gloo(world):
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


def test_single_process_rows_match_brute_force():
    train, synth, holdout = _data()
    from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
    rows = sharded_nearest_records(ShardComm(False), NumpyKernels(), train, synth, holdout)
    a, b, h = synth.double().numpy(), train.double().numpy(), holdout.double().numpy()
    d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    srt = np.sort(d, axis=1)
    np.testing.assert_allclose(rows["dcr"], srt[:, 0], rtol=1e-6)
    np.testing.assert_allclose(rows["second"], srt[:, 1], rtol=1e-6)
    assert np.array_equal(rows["match"], d.argmin(1))
    bb = np.sqrt(((b[:, None, :] - b[None, :, :]) ** 2).sum(-1)) + np.diag(np.full(37, np.inf))
    np.testing.assert_allclose(rows["real_nn"], bb.min(1), rtol=1e-6)
    np.testing.assert_allclose(rows["dcr_holdout"], np.sqrt(((a[:, None, :] - h[None, :, :]) ** 2).sum(-1)).min(1), rtol=1e-6)
