"""CPU: the host side of precision / recall / density / coverage (osteosarcoma_diffusionmodel_amd/validation.py) -- ``prdc_summary``
on hand-written counts and against the definitions evaluated directly in fp64, and the argument errors of
``BiologicalValidator.fidelity_diversity`` that are raised before any device call (the GPU tests run the kernels)."""
import numpy as np
import pytest

from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, prdc_summary

KEYS = ["prdc_precision", "prdc_recall", "prdc_density", "prdc_coverage", "prdc_k"]


def _dist(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def _radius(a, k):
    d = _dist(a, a)
    d[np.arange(len(a)), np.arange(len(a))] = np.inf          # the row itself is no neighbour
    return np.sort(d, axis=1)[:, k - 1]


def _rows(x, y, k):
    """The per-row counts of prdc_summary's docstring by brute force."""
    rx, ry, d = _radius(x, k), _radius(y, k), _dist(x, y)     # d[i][j] = d(x_i, y_j)
    return {"synth_in_real_balls": (d <= rx[:, None]).sum(0), "real_in_synth_balls": (d <= ry[None, :]).sum(1),
            "real_ball_synth": (d <= rx[:, None]).sum(1)}


def _direct(x, y, k):
    """Naeem et al.'s four definitions, written out pair by pair."""
    rx, ry, d = _radius(x, k), _radius(y, k), _dist(x, y)
    n, m = len(x), len(y)
    precision = np.mean([any(d[i, j] <= rx[i] for i in range(n)) for j in range(m)])
    density = sum(sum(d[i, j] <= rx[i] for i in range(n)) for j in range(m)) / (k * m)
    recall = np.mean([any(d[i, j] <= ry[j] for j in range(m)) for i in range(n)])
    coverage = np.mean([any(d[i, j] <= rx[i] for j in range(m)) for i in range(n)])
    return {"prdc_precision": float(precision), "prdc_recall": float(recall), "prdc_density": float(density),
            "prdc_coverage": float(coverage), "prdc_k": k}


def test_prdc_summary_hand_computed():
    rows = {"synth_in_real_balls": np.array([0, 2, 1, 0]), "real_in_synth_balls": np.array([1, 0, 0]),
            "real_ball_synth": np.array([0, 0, 3]), "real_radius": np.ones(3)}       # further keys are ignored
    s = prdc_summary(rows, 2)
    assert list(s) == KEYS
    assert s["prdc_precision"] == 0.5 and s["prdc_density"] == 3 / (2 * 4)
    assert s["prdc_recall"] == 1 / 3 and s["prdc_coverage"] == 1 / 3 and s["prdc_k"] == 2
    assert all(type(s[k]) is float for k in KEYS[:4]) and type(s["prdc_k"]) is int
    with pytest.raises(ValueError):
        prdc_summary(rows, 0)
    with pytest.raises(ValueError):
        prdc_summary({**rows, "real_ball_synth": np.array([0, 0])}, 2)
    with pytest.raises(ValueError):
        prdc_summary({**rows, "synth_in_real_balls": np.zeros(0, dtype=np.int64)}, 2)


@pytest.mark.parametrize("k", [1, 3, 5])
def test_prdc_summary_vs_direct_definitions(k):
    rs = np.random.default_rng(11 + k)
    x = rs.standard_normal((41, 6)).astype(np.float32)
    y = (rs.standard_normal((29, 6)) * 0.7 + 0.4).astype(np.float32)
    got, ref = prdc_summary(_rows(x, y, k), k), _direct(x, y, k)
    assert got == ref
    assert 0 < got["prdc_precision"] < 1 or 0 < got["prdc_recall"] < 1       # not a vacuous comparison


def test_identical_and_collapsed_cohorts():
    rs = np.random.default_rng(3)
    n, k = 50, 3
    x = rs.standard_normal((n, 5)).astype(np.float32)
    same = prdc_summary(_rows(x, x.copy(), k), k)
    assert same["prdc_precision"] == 1.0 and same["prdc_recall"] == 1.0 and same["prdc_coverage"] == 1.0
    assert same["prdc_density"] >= 1.0 / k                     # every copy lies in its original's ball at the least
    # mode collapse: the synthetic cohort is one real row, repeated -- every synthetic row is realistic, the cohort covers nothing
    y = np.repeat(x[7:8], 20, axis=0)
    rows = _rows(x, y, k)
    col = prdc_summary(rows, k)
    assert col["prdc_precision"] == 1.0
    assert col["prdc_recall"] == 1 / n                         # the synthetic radii are 0: only x_7 itself lies in a synthetic ball
    has7 = int((_dist(x, x[7:8])[:, 0] <= _radius(x, k)).sum())              # real rows with x_7 inside their own ball, x_7 included
    assert col["prdc_coverage"] == has7 / n and 1 / n <= col["prdc_coverage"] <= 0.25
    assert col == _direct(x, y, k)


def test_fidelity_diversity_argument_errors_need_no_device():
    val = BiologicalValidator({"evaluation": {}}, device="cuda:0")
    x = np.zeros((9, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="same features"):
        val.fidelity_diversity(x, x[:, :3])
    with pytest.raises(ValueError, match="same features"):
        val.fidelity_diversity(x, np.zeros(9, dtype=np.float32))
    with pytest.raises(ValueError, match="more than k"):
        val.fidelity_diversity(x[:5], x, k=5)
    with pytest.raises(ValueError, match="more than k"):
        val.fidelity_diversity(x, x[:3], k=3)
    for k in (0, 17):
        with pytest.raises(ValueError, match=r"\[1, 16\]"):
            val.fidelity_diversity(x, x, k=k)
    sharded = BiologicalValidator({"evaluation": {}}, device="cuda:0", sharded=True)
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.fidelity_diversity(x, x)
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.fidelity_diversity(x, x[:, :3])                # said first, whatever the arguments
