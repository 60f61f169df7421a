"""Float64 restatement of the two kernels behind pca.DevicePCA (osd_val_pca_project, osd_val_pca_backproject), a ``NumpyKernels``
stand-in with the semantics of validation.DeviceKernels, a plain float64 subspace driver that shares no code with the package, and
the planted cohorts the PCA tests share.  Everything here evaluates the SAME fp32 inputs the device sees, in double, so a difference
to the device is the device's rounding alone; the float64 pipeline is the package's own host code (pca.DevicePCA,
pca.embedding_rows) over these kernels."""
import functools

import numpy as np
import torch

from marginal_helpers import NumpyKernels as _MarginalKernels

U53 = 2.0 ** -53
PLANTED_SD = np.array([6.0, 5.0, 4.0, 3.0, 2.5])
PLANTED_OFFSET = 3.0


def _f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _d(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def centred64(x, center, scale=None):
    """u = (x - center) * scale in float64 from the fp32 values of x; ``scale`` None: 1."""
    u = _f64(x) - _d(center)
    return u if scale is None else u * _d(scale)


def project64(x, center, scale, V):
    """(Z float64 [rows, l], norm2 float64 [rows]): u V and the rows' squared norms."""
    u = centred64(x, center, scale)
    return u @ _d(V), (u * u).sum(1)


def backproject64(x, center, scale, Z):
    """W float64 [D, l] = u^T Z."""
    return centred64(x, center, scale).T @ _d(Z)


def project_bound(x, center, scale, V):
    """(bz [rows, l], bn [rows]): sum_c |u_rc V_cj| and sum_c u_rc^2 -- what the kernels' error bounds are multiples of."""
    u = np.abs(centred64(x, center, scale))
    return u @ np.abs(_d(V)), (u * u).sum(1)


def backproject_bound(x, center, scale, Z):
    return np.abs(centred64(x, center, scale)).T @ np.abs(_d(Z))


class NumpyKernels(_MarginalKernels):
    """``col_moments64``, ``pca_project`` and ``pca_backproject`` with the semantics of validation.DeviceKernels on CPU tensors, in
    double, beside the ``marginals`` it inherits."""

    @staticmethod
    def col_moments64(t, center=None):
        if int(t.shape[0]) == 0:
            return np.zeros(int(t.shape[1])), np.zeros(int(t.shape[1]))
        d = _f64(t) - (0.0 if center is None else _f64(center))
        return d.sum(0), (d * d).sum(0)

    @staticmethod
    def pca_project(x, center, scale, V, norm2=False):
        z, n2 = project64(x, center, scale, V)
        return torch.from_numpy(z), (torch.from_numpy(n2) if norm2 else None)

    @staticmethod
    def pca_backproject(x, center, scale, Z):
        return torch.from_numpy(backproject64(x, center, scale, Z))


def subspace64(x, V0, k, max_iter=100, tol=1e-9):
    """Block subspace iteration with Rayleigh-Ritz on the float64 copy of ``x`` from the basis ``V0`` [D, l], written out plainly:
    a dict of ``eigenvalues`` (lambda / (n - 1), [k]), ``components`` ([k, D], the entry of largest magnitude of every row
    positive), ``n_iter``, ``converged``, ``residual`` and ``mean``."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.mean(0)
    u = x - mean
    V = np.array(V0, dtype=np.float64)
    for it in range(1, max_iter + 1):
        W = u.T @ (u @ V)
        T = V.T @ W
        lam, S = np.linalg.eigh(0.5 * (T + T.T))
        lam, S = lam[::-1], S[:, ::-1]
        resid = np.linalg.norm(W @ S - (V @ S) * lam, axis=0) / lam[0]
        done = resid[:k].max() <= tol
        if done or it == max_iter:
            break
        V = np.linalg.qr(W)[0]
    comps = (V @ S)[:, :k].T.copy()
    for row in comps:
        if row[np.argmax(np.abs(row))] < 0:
            row *= -1.0
    return {"eigenvalues": lam[:k] / (n - 1), "components": comps, "n_iter": it, "converged": bool(done),
            "residual": float(resid[:k].max()), "mean": mean}


@functools.lru_cache(maxsize=None)
def _basis(D, rotate):
    return np.linalg.qr(np.random.RandomState(11 if rotate else 7).randn(D, 5))[0]


@functools.lru_cache(maxsize=None)
def cohort(n, D, k=5, seed=0, shrink=1.0, noise=1.0, rotate=False):
    """float32 [n, D]: k <= 5 planted directions (the first k columns of a fixed orthonormal D x 5 basis; ``rotate`` draws another
    basis) with score sd (6, 5, 4, 3, 2.5) * shrink, isotropic noise of sd ``noise`` and the offset 3.0.  Shared between tests: copy
    before changing a value."""
    rs = np.random.RandomState(1000 + seed)
    scores = rs.randn(n, k) * (PLANTED_SD[:k] * shrink)
    x = scores @ _basis(D, bool(rotate))[:, :k].T + noise * rs.randn(n, D) + PLANTED_OFFSET
    return x.astype(np.float32)


SAMPLERS = {"faithful": {}, "shrink": {"shrink": 0.5}, "noise": {"noise": 1.3}, "rotate": {"rotate": True}}


def planted_pair(kind, n_real=600, n_synth=900, D=130):
    """(real, synthetic) float32 cohorts of one of the four planted samplers."""
    return cohort(n_real, D, 5, 1), cohort(n_synth, D, 5, 2, **SAMPLERS[kind])


def check_separations(kind, out, k=5):
    """The separations the planted samplers must show, on any kernels."""
    ratios = np.array([out[f"pca_variance_ratio_{i + 1}"] for i in range(k)])
    if kind == "faithful":
        assert ((ratios >= 0.8) & (ratios <= 1.2)).all() and out["pca_offmanifold_share"] < 0.05 and out["pca_subspace_cos_min"] > 0.9
    elif kind == "shrink":
        assert (ratios < 0.5).all() and out["pca_offmanifold_share"] < 0.05
    elif kind == "noise":
        assert out["pca_offmanifold_share"] > 0.5 and ((ratios >= 0.8) & (ratios <= 1.3)).all()
    else:
        assert out["pca_subspace_cos_min"] < 0.2
