"""CPU: the host side of subtype fidelity -- ``validation.subtype_summary`` on hand-made counts, and ``cluster.kmeans`` /
``cluster.subtype_rows`` driven by the float64 NumPy kernels of tests/cluster_helpers.py (the device kernels are tested in
tests/test_gpu_cluster.py); plus the new entry point's place in the header and the ctypes table."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from osteosarcoma_diffusionmodel_amd import cluster as CL
from osteosarcoma_diffusionmodel_amd.parallel import ShardComm
from osteosarcoma_diffusionmodel_amd.validation import DeviceKernels, subtype_summary
from cluster_helpers import NumpyKernels, blobs, centred, label_sums64

ROOT = Path(__file__).resolve().parent.parent


def _rows(n, m, rd2=None, sd2=None, centroids=None, synth_sums=None, **more):
    n, m = np.asarray(n, dtype=np.int64), np.asarray(m, dtype=np.int64)
    K = len(n)
    centroids = np.zeros((K, 2)) if centroids is None else np.asarray(centroids, dtype=np.float64)
    rows = {"k": K, "inertia": 1.5, "iterations": 3, "converged": True, "real_counts": n, "synth_counts": m,
            "real_d2_sums": n.astype(np.float64) if rd2 is None else np.asarray(rd2, dtype=np.float64),
            "synth_d2_sums": m.astype(np.float64) if sd2 is None else np.asarray(sd2, dtype=np.float64),
            "centroids_centered": centroids,
            "synth_sums": centroids * m[:, None] if synth_sums is None else np.asarray(synth_sums, dtype=np.float64)}
    rows.update(more)
    return rows


# ---- subtype_summary ------------------------------------------------------------------------------------------------------------
def test_summary_identical_cohorts():
    out = subtype_summary(_rows([50, 30, 20], [50, 30, 20], rd2=[100.0, 45.0, 10.0], sd2=[100.0, 45.0, 10.0]))
    assert out["subtype_js_divergence"] == 0.0 and out["subtype_tv_distance"] == 0.0
    assert out["subtype_min_share_ratio"] == 1.0 and out["subtype_missing"] == 0
    assert [out[f"subtype_dispersion_ratio_{k}"] for k in range(3)] == [1.0, 1.0, 1.0] and out["subtype_dispersion_ratio_min"] == 1.0
    assert out["subtype_centroid_shift_max"] == 0.0
    assert (out["subtype_k"], out["subtype_inertia"], out["subtype_iterations"], out["subtype_converged"]) == (3, 1.5, 3, True)
    assert [out[f"subtype_real_share_{k}"] for k in range(3)] == [0.5, 0.3, 0.2]
    # the same shares at another cohort size
    out = subtype_summary(_rows([50, 30, 20], [100, 60, 40]))
    assert out["subtype_js_divergence"] == 0.0 and out["subtype_tv_distance"] == 0.0 and out["subtype_min_share_ratio"] == 1.0


def test_summary_missing_subtype_and_shares():
    out = subtype_summary(_rows([40, 36, 18, 6], [60, 40, 0, 0]))
    assert out["subtype_missing"] == 2 and out["subtype_min_share_ratio"] == 0.0
    out = subtype_summary(_rows([40, 36, 18, 6], [50, 30, 0, 20]))
    assert out["subtype_missing"] == 1 and out["subtype_min_share_ratio"] == 0.0
    p, q = np.array([0.4, 0.36, 0.18, 0.06]), np.array([0.5, 0.3, 0.0, 0.2])
    assert out["subtype_tv_distance"] == pytest.approx(0.5 * np.abs(p - q).sum(), rel=1e-15)
    mix = 0.5 * (p + q)
    js = 0.5 * (p * np.log2(p / mix)).sum() + 0.5 * (q[q > 0] * np.log2(q[q > 0] / mix[q > 0])).sum()
    assert out["subtype_js_divergence"] == pytest.approx(js, rel=1e-14) and 0.0 < js < 1.0
    assert math.isnan(out["subtype_dispersion_ratio_2"]) and math.isnan(out["subtype_centroid_shift_2"])
    # an over-produced subtype is no missing one
    out = subtype_summary(_rows([40, 40, 20], [10, 10, 80]))
    assert out["subtype_missing"] == 0 and out["subtype_min_share_ratio"] == pytest.approx(0.25, rel=1e-15)


def test_summary_disjoint_supports_give_js_exactly_one():
    for n, m in (([7, 3, 0, 0], [0, 0, 1, 12]), ([1, 0], [0, 1]), ([33, 0, 34], [0, 3, 0])):
        out = subtype_summary(_rows(n, m))
        assert out["subtype_js_divergence"] == 1.0 and out["subtype_tv_distance"] == pytest.approx(1.0, rel=1e-15)
        assert out["subtype_missing"] == sum(v > 0 for v in n) and out["subtype_min_share_ratio"] == 0.0
        assert math.isnan(out["subtype_dispersion_ratio_min"]) and math.isnan(out["subtype_centroid_shift_max"])


def test_summary_nan_rules_and_ratios():
    # subtype 1: no synthetic row; subtype 2: no real row; subtype 3: real rows all ON the centroid (dispersion 0)
    out = subtype_summary(_rows([10, 5, 0, 4], [20, 0, 3, 8], rd2=[40.0, 10.0, 0.0, 0.0], sd2=[20.0, 0.0, 9.0, 16.0],
                                centroids=[[1.0, 0.0], [0.0, 1.0], [2.0, 2.0], [3.0, 3.0]],
                                synth_sums=[[20.0 + 20 * 1.2, 20 * 1.6], [0.0, 0.0], [6.0, 6.0], [24.0, 24.0]]))
    assert out["subtype_dispersion_ratio_0"] == pytest.approx((20.0 / 20) / (40.0 / 10), rel=1e-15)
    for k in (1, 2, 3):
        assert math.isnan(out[f"subtype_dispersion_ratio_{k}"]) and math.isnan(out[f"subtype_centroid_shift_{k}"])
    assert out["subtype_dispersion_ratio_min"] == out["subtype_dispersion_ratio_0"]
    # mean of the synthetic rows of 0 = (2.2, 1.6): 2 away from (1, 0); real root mean d2 = 2
    assert out["subtype_centroid_shift_0"] == pytest.approx(1.0, rel=1e-12) and out["subtype_centroid_shift_max"] == out["subtype_centroid_shift_0"]
    assert out["subtype_missing"] == 1 and out["subtype_min_share_ratio"] == 0.0
    assert out["subtype_real_share_2"] == 0.0 and out["subtype_synth_share_2"] == pytest.approx(3 / 31)
    # the minimum is over the finite ratios only
    out = subtype_summary(_rows([10, 10], [10, 10], rd2=[10.0, 10.0], sd2=[0.9, 20.0]))
    assert out["subtype_dispersion_ratio_min"] == pytest.approx(0.09, rel=1e-15) and out["subtype_dispersion_ratio_1"] == 2.0


def test_summary_condition_gap_over_subtypes_both_populate():
    rows = _rows([10, 5, 4], [20, 0, 8], condition_names=["met", "age"],
                 real_condition_sums=[[5.0, 600.0], [5.0, 100.0], [1.0, 200.0]],
                 synth_condition_sums=[[4.0, 1300.0], [0.0, 0.0], [6.0, 400.0]])
    out = subtype_summary(rows)
    assert out["subtype_condition_gap_met"] == pytest.approx(max(abs(0.5 - 0.2), abs(0.25 - 0.75)), rel=1e-15)
    assert out["subtype_condition_gap_age"] == pytest.approx(max(abs(60.0 - 65.0), abs(50.0 - 50.0)), rel=1e-15)
    assert "subtype_condition_gap_met" not in subtype_summary(_rows([1], [1]))
    with pytest.raises(ValueError):
        subtype_summary(_rows([1, 2], [0, 0]))


def test_renumbering_with_tied_counts():
    assert CL.renumber_order([5, 9, 5, 9, 1]).tolist() == [1, 3, 0, 2, 4]
    assert CL.renumber_order([3, 3, 3]).tolist() == [0, 1, 2]
    assert CL.renumber_order([0, 7]).tolist() == [1, 0]


# ---- kmeans on the NumPy kernels ------------------------------------------------------------------------------------------------
def _t(x):
    return torch.from_numpy(np.array(x, dtype=np.float32))


def test_kmeans_pp_centres_are_rows_one_per_separated_blob():
    x, truth, _ = blobs(300, 6, 3, 40.0)      # a second centre inside a chosen blob has a chance of about 1e-3 per draw
    for seed in range(6):
        idx = CL.kmeans_pp_indices(_t(x), 3, np.random.default_rng(seed), NumpyKernels())
        assert len(set(idx)) == 3 and all(0 <= i < 300 for i in idx)
        assert idx[0] == int(np.random.default_rng(seed).integers(300))
        assert sorted(truth[idx].tolist()) == [0, 1, 2], (seed, idx)
        fit = CL.kmeans(_t(x), 3, seed=seed, max_iter=1, kernels=NumpyKernels())      # one pass: the centroids are still the centres
        assert np.array_equal(fit.centroids.numpy(), x[idx]) and not fit.converged and fit.iterations == 1


def test_kmeans_recovers_separated_blobs_and_is_reproducible():
    x, truth, _ = blobs(300, 6, 3, 8.0)
    a = CL.kmeans(_t(x), 3, seed=5, kernels=NumpyKernels())
    b = CL.kmeans(_t(x), 3, seed=5, kernels=NumpyKernels())
    assert a.converged and a.empty == [] and a.iterations >= 2
    assert torch.equal(a.labels, b.labels) and torch.equal(a.centroids, b.centroids) and a.inertia == b.inertia and a.iterations == b.iterations
    lab = a.labels.numpy()
    assert a.labels.dtype == torch.int32 and a.centroids.dtype == torch.float32 and tuple(a.centroids.shape) == (3, 6)
    for k in range(3):                                     # a cluster is a blob
        assert len(set(truth[lab == k].tolist())) == 1
    assert np.array_equal(a.counts, np.bincount(lab, minlength=3)) and a.counts.dtype == np.int64
    assert a.inertia == pytest.approx(float(a.d2.double().sum()), rel=1e-15)
    sums, counts, _ = label_sums64(x, lab, 3)
    assert np.array_equal(a.centroids.numpy(), (sums / counts[:, None]).astype(np.float32))      # the mean, rounded once


def test_kmeans_fewer_distinct_rows_than_clusters():
    x = np.tile(np.array([[1.0, -2.0, 0.5]], dtype=np.float32), (7, 1))
    first = int(np.random.default_rng(0).integers(7))
    idx = CL.kmeans_pp_indices(_t(x), 3, np.random.default_rng(0), NumpyKernels())
    assert idx == [first] + [j for j in range(7) if j != first][:2]                   # total d2 = 0: the smallest unchosen rows
    fit = CL.kmeans(_t(x), 3, seed=0, kernels=NumpyKernels())
    assert fit.converged and fit.iterations == 2 and fit.inertia == 0.0
    assert fit.counts.tolist() == [7, 0, 0] and fit.empty == [1, 2]                   # ties go to the smallest index
    assert np.array_equal(fit.centroids.numpy(), x[:3]) and np.isfinite(fit.centroids.numpy()).all()
    two = np.concatenate([x[:4], x[:3] + 1.0])
    fit = CL.kmeans(_t(two), 4, seed=3, kernels=NumpyKernels())
    assert fit.converged and fit.inertia == 0.0 and sorted(fit.counts.tolist()) == [0, 0, 3, 4]


def test_kmeans_empty_cluster_keeps_its_centroid():
    x, _, _ = blobs(120, 5, 2, 6.0)
    far = np.full(5, 1.0e3, dtype=np.float32)
    init = np.stack([x[0], far, x[1]])
    fit = CL.kmeans(_t(x), 3, init=init, kernels=NumpyKernels())
    assert fit.converged and fit.empty == [1] and fit.counts[1] == 0 and fit.counts.sum() == 120
    assert np.array_equal(fit.centroids.numpy()[1], far)
    assert not np.array_equal(fit.centroids.numpy()[0], x[0])


def test_kmeans_explicit_init_is_used_as_given():
    x, _, _ = blobs(200, 4, 3, 1.0)
    init = np.array(x[[10, 20, 30]]) + np.float32(0.25)
    k = NumpyKernels()
    fit = CL.kmeans(_t(x), 3, init=init, max_iter=1, n_init=5, seed=9, kernels=k)
    assert np.array_equal(fit.centroids.numpy(), init) and k.calls == 1               # no restart, no draw
    d = ((x.astype(np.float64)[:, None, :] - init.astype(np.float64)[None]) ** 2).sum(2)
    assert np.array_equal(fit.labels.numpy(), d.argmin(1)) and fit.iterations == 1 and not fit.converged
    full = CL.kmeans(_t(x), 3, init=torch.from_numpy(init), kernels=NumpyKernels())
    assert full.converged and full.iterations > 2
    capped = CL.kmeans(_t(x), 3, init=init, max_iter=full.iterations - 1, kernels=NumpyKernels())
    assert not capped.converged and capped.iterations == full.iterations - 1
    d2 = ((x.astype(np.float64) - capped.centroids.numpy().astype(np.float64)[capped.labels.numpy()]) ** 2).sum(1)
    assert np.allclose(capped.d2.numpy(), d2, rtol=1e-12)                             # labels and d2 belong to the returned centroids
    for bad in (dict(init=init[:2]), dict(init="random"), dict(max_iter=0), dict(n_init=0)):
        with pytest.raises(ValueError):
            CL.kmeans(_t(x), 3, kernels=NumpyKernels(), **bad)
    for K in (0, 65, 201):
        with pytest.raises(ValueError):
            CL.kmeans(_t(x), K, kernels=NumpyKernels())


def test_kmeans_n_init_keeps_the_lowest_inertia():
    x, _, _ = blobs(240, 3, 6, 2.0)
    single = [CL.kmeans(_t(x), 6, seed=4 + r, kernels=NumpyKernels()) for r in range(5)]
    inertias = [f.inertia for f in single]
    assert len(set(inertias)) > 1                                                     # the restarts do not all agree
    best = CL.kmeans(_t(x), 6, seed=4, n_init=5, kernels=NumpyKernels())
    r = int(np.argmin(inertias))                                                      # the earliest of the lowest
    assert best.inertia == inertias[r] and torch.equal(best.labels, single[r].labels) and torch.equal(best.centroids, single[r].centroids)


# ---- the subtype pipeline in double ---------------------------------------------------------------------------------------------
def test_subtype_rows_on_planted_cohorts():
    x, truth, mu = blobs(400, 12, 3, 4.0)
    rs = np.random.default_rng(1)
    t2 = rs.choice(3, size=500, p=np.bincount(truth, minlength=3) / 400.0)
    y = (mu[t2] + rs.standard_normal((500, 12))).astype(np.float32)
    rows = CL.subtype_rows(ShardComm(False), NumpyKernels(), _t(x), _t(y), 3, seed=0, n_init=2)
    out = subtype_summary(rows)
    n = rows["real_counts"]
    assert n.tolist() == sorted(np.bincount(truth, minlength=3).tolist(), reverse=True)      # renumbered by descending real count
    assert np.array_equal(np.bincount(rows["real_labels"], minlength=3), n) and rows["synth_counts"].sum() == 500
    assert out["subtype_missing"] == 0 and out["subtype_js_divergence"] < 0.01 and out["subtype_converged"]
    assert all(0.8 < out[f"subtype_dispersion_ratio_{k}"] < 1.25 for k in range(3)) and out["subtype_centroid_shift_max"] < 0.3
    assert np.allclose(rows["centroids"], np.stack([x[rows["real_labels"] == k].astype(np.float64).mean(0) for k in range(3)]), atol=1e-5)
    # the sampler loses the real cohort's smallest subtype and inverts a binary condition inside the largest
    gone = int(np.argmin(np.bincount(truth, minlength=3)))
    keep = t2 != gone
    rc = (rs.random(400) < 0.3).astype(np.float32)[:, None]
    big = rows["synth_labels"][keep] == 0
    sc = (rs.random(int(keep.sum())) < 0.3).astype(np.float32)
    sc[big] = 1.0 - sc[big]
    rows2 = CL.subtype_rows(ShardComm(False), NumpyKernels(), _t(x), _t(y[keep]), 3, conditions=(_t(rc), _t(sc[:, None])), names=["met"],
                            seed=0, n_init=2)
    out2 = subtype_summary(rows2)
    assert out2["subtype_missing"] == 1 and out2["subtype_min_share_ratio"] == 0.0 and rows2["synth_counts"][2] == 0
    r0 = rc[rows2["real_labels"] == 0, 0].astype(np.float64).mean()
    s0 = sc[rows2["synth_labels"] == 0].astype(np.float64).mean()
    assert out2["subtype_condition_gap_met"] == pytest.approx(abs(r0 - s0), rel=1e-12) and out2["subtype_condition_gap_met"] > 0.25


# ---- the entry point's place in the C ABI ---------------------------------------------------------------------------------------
def test_label_sums_is_declared_bound_and_exported():
    from osteosarcoma_diffusionmodel_amd import _lib as L
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "osdiff.h").read_text(), flags=re.S)
    assert re.search(r"\bosd_val_label_sums\s*\(", header)
    assert "osd_val_label_sums" in L.exported_symbols() and hasattr(L.lib(), "osd_val_label_sums")
    assert L.lib().osd_version() == 100
    assert callable(getattr(DeviceKernels, "label_sums"))


def test_centred_helper_matches_the_pipeline():
    x, _, _ = blobs(50, 4, 2, 1.0)
    mean = (label_sums64(x, np.zeros(50, dtype=np.int64), 1)[0][0] / 50.0).astype(np.float32)
    assert np.array_equal(centred(x), x - mean)
