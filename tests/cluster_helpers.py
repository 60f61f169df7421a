"""Float64 restatement of the two kernels behind cluster.kmeans (osd_val_nearest against K centroids, osd_val_label_sums) and the blob
cohorts the cluster tests share.  Everything here evaluates the SAME fp32 inputs the device sees, in double, so a difference to the
device is the device's rounding alone; the float64 pipeline is the package's own host code (cluster.lloyd, cluster.subtype_rows) over
these kernels."""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24


def _f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def distances64(x, c):
    """float64 [N, K]: squared distances of the fp32 rows of x to the fp32 rows of c, by differences."""
    x, c = _f64(x), _f64(c)
    out = np.empty((x.shape[0], c.shape[0]))
    for k in range(c.shape[0]):
        d = x - c[k]
        out[:, k] = (d * d).sum(1)
    return out


def ambiguity_bound(x, c):
    """float64 [N]: 2 (D + 4) 2^-24 (|x|^2 + max |c|^2) -- the worst case of the fp32 expanded form |x|^2 + |c|^2 - 2 x.c the Gram
    pass ranks the centroids by.  A row whose float64 margin d2_(2) - d2_(1) is below it may go to either of its two nearest."""
    x, c = _f64(x), _f64(c)
    return 2.0 * (x.shape[1] + 4) * EPS * ((x * x).sum(1) + (c * c).sum(1).max())


def margins(x, c):
    """(labels int64 [N], d2 float64 [N], margin float64 [N]): nearest centroid (ties to the smallest index), its squared distance and
    the distance of the runner-up minus it (+inf with one centroid)."""
    d = distances64(x, c)
    labels = d.argmin(1)
    best = d[np.arange(d.shape[0]), labels]
    if d.shape[1] < 2:
        return labels, best, np.full(d.shape[0], np.inf)
    return labels, best, np.partition(d, 1, axis=1)[:, 1] - best


class NumpyKernels:
    """``nearest`` and ``label_sums`` with the semantics of validation.DeviceKernels on CPU tensors, in double.  ``min_ratio`` is the
    smallest margin / ambiguity bound any ``nearest`` call has seen since the object was made (+inf before the first): the device may
    differ from this reference only where it is small."""

    def __init__(self):
        self.min_ratio = np.inf
        self.calls = 0

    def nearest(self, q, r, exclude=None):
        assert exclude is None
        labels, d2, margin = margins(q, r)
        self.calls += 1
        if r.shape[0] > 1:
            self.min_ratio = min(self.min_ratio, float((margin / ambiguity_bound(q, r)).min()))
        return torch.from_numpy(d2), torch.from_numpy(labels.astype(np.int32))

    @staticmethod
    def label_sums(t, labels, K, value=None):
        return tuple(None if a is None else torch.from_numpy(a) for a in label_sums64(t, labels, K, value))


def label_sums64(t, labels, K, value=None):
    """(sums float64 [K, D], counts int64 [K], value sums float64 [K] or None) of the fp32 rows of t; labels outside [0, K) add to
    nothing."""
    t = _f64(t)
    labels = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels).astype(np.int64)
    sums, counts = np.zeros((K, t.shape[1])), np.zeros(K, dtype=np.int64)
    vs = None if value is None else np.zeros(K)
    for k in range(K):
        sel = labels == k
        sums[k] = t[sel].sum(0)
        counts[k] = int(sel.sum())
        if value is not None:
            vs[k] = _f64(value)[sel].sum()
    return sums, counts, vs


@functools.lru_cache(maxsize=None)
def blobs(n, D, K, sep, seed=0):
    """(x float32 [n, D], truth int64 [n], mu float64 [K, D]): K Gaussian blobs with centres mu = sep N(0, 1), unit noise and
    Dirichlet(3) weights, every blob with at least one row (the first K rows are one of each).  Shared between tests: copy before
    changing a value."""
    rs = np.random.default_rng(104729 * n + 131 * D + 7 * K + 1000003 * seed)
    mu = sep * rs.standard_normal((K, D))
    w = rs.dirichlet(np.full(K, 3.0))
    truth = rs.choice(K, size=n, p=w)
    truth[:K] = np.arange(K)
    x = (mu[truth] + rs.standard_normal((n, D))).astype(np.float32)
    return x, truth.astype(np.int64), mu


def centred(x):
    """x minus its fp32 column means, as subtype_fidelity does before it clusters."""
    x = np.asarray(x, dtype=np.float32)
    return x - (x.astype(np.float64).mean(0)).astype(np.float32)
