"""Principal components of a device-resident cohort by block subspace iteration, and the embedding-fidelity figures built on them
(DESIGN.md section 3.33).  An iteration is two library calls -- ``kernels.pca_project`` (``osd_val_pca_project``: Z = U V and the
rows' squared norms) and ``kernels.pca_backproject`` (``osd_val_pca_backproject``: W = U^T Z), U the centred (and optionally
standardised) cohort in double -- and everything else here is host logic over their results: a QR and a symmetric l x l
eigenproblem per iteration, l <= 32.  Only D x l doubles cross the bus per iteration, and neither the D x D Gram matrix nor its
eigen-decomposition is ever formed.  ``kernels`` is any object with ``col_moments64``, ``pca_project`` and ``pca_backproject``
(``validation.DeviceKernels``, or a float64 NumPy stand-in in the CPU tests), the way ``cluster.kmeans`` is driven.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .parallel import ShardComm

MAX_DIRS = 32                     # OSD_PCA_MAX_DIRS: the directions of one osd_val_pca_* call
_PARAMS = ("n_components", "oversample", "max_iter", "tol", "standardize", "seed")
_ARRAYS = ("mean_", "scale_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_")
_NUMBERS = ("n_samples_", "n_iter_", "converged_", "max_residual_", "constant_features_", "total_variance_")


def _cohort(x, kernels):
    """(fp32 [rows, D] tensor, kernels): ``x`` (a tensor, a ``DeviceFrame`` / DataFrame, or a host array) where the kernels read it
    -- on the ROCm device with the default ``DeviceKernels``, as it is with a stand-in."""
    if hasattr(x, "values") and not isinstance(x, torch.Tensor):
        x = x.values
    if kernels is None:
        from .validation import DeviceKernels, _dev
        device = x.device if isinstance(x, torch.Tensor) and x.is_cuda else torch.device("cuda", torch.cuda.current_device())
        t = x if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 else _dev(x, device)
        kernels = DeviceKernels(t.device)
    else:
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        t = t.to(torch.float32)
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError("x must be a [rows, features] matrix")
    return t, kernels


def svd_flip_rows(components: np.ndarray) -> np.ndarray:
    """Every row's entry of largest absolute value made positive: sklearn's ``svd_flip(u_based_decision=False)``."""
    c = np.array(components, dtype=np.float64, copy=True)
    if c.size:
        pick = np.argmax(np.abs(c), axis=1)
        signs = np.sign(c[np.arange(c.shape[0]), pick])
        signs[signs == 0] = 1.0
        c *= signs[:, None]
    return c


class DevicePCA:
    """The top ``n_components`` principal directions of the rows of a cohort, with sklearn's attribute names.

    ``fit`` takes the column means (and with ``standardize=True`` the sample standard deviations: a constant column gets scale 0
    and is counted in ``constant_features_``) in float64 from two ``col_moments64`` passes, then iterates on a block of
    l = min(n_components + oversample, D, 32) directions, from the Q of a QR of ``RandomState(seed).randn(D, l)``:
    W = U^T (U V) by the two calls, T = (V^T W + W^T V) / 2, ``eigh(T)`` gives the Ritz pairs (lambda_j, V S_j), the residual of pair
    j is ||W S_j - lambda_j V S_j|| / lambda_1, and the fit stops when the largest residual over the first ``n_components`` pairs is
    at most ``tol``; otherwise V becomes the Q of a QR of W.  A fit that reaches ``max_iter`` is not an error: ``converged_`` is
    False and the last Ritz pairs are kept."""

    def __init__(self, n_components: int = 10, oversample: int = 8, max_iter: int = 100, tol: float = 1e-9, standardize: bool = False,
                 seed: int = 0):
        self.n_components, self.oversample, self.max_iter = int(n_components), int(oversample), int(max_iter)
        self.tol, self.standardize, self.seed = float(tol), bool(standardize), int(seed)
        if not 1 <= self.n_components <= MAX_DIRS:
            raise ValueError(f"n_components must lie in [1, {MAX_DIRS}], got {self.n_components}")
        if self.oversample < 0 or self.max_iter < 1 or not self.tol >= 0.0:
            raise ValueError("oversample >= 0, max_iter >= 1 and tol >= 0 are needed")
        self.mean_ = None

    # -- the fit ------------------------------------------------------------------------------------------------------------------
    def initial_basis(self, D: int) -> np.ndarray:
        """V_0 float64 [D, l]: the Q of a QR of ``RandomState(seed).randn(D, l)``."""
        l = min(self.n_components + self.oversample, int(D), MAX_DIRS)
        return np.linalg.qr(np.random.RandomState(self.seed).randn(int(D), l))[0]

    def fit(self, x, comm: Optional[ShardComm] = None, kernels=None) -> "DevicePCA":
        """Fit on ``x`` (an fp32 device tensor, a ``DeviceFrame`` or a host array; finite values).  With an active ``comm``, ``x`` is
        this rank's rows: the moments, W and the norm totals are summed over the ranks, an empty shard contributes nothing, and
        every rank ends with the same attributes."""
        t, k = _cohort(x, kernels)
        comm = comm if comm is not None else ShardComm(False)
        D, k_want = int(t.shape[1]), self.n_components
        if k_want > D:
            raise ValueError(f"n_components = {k_want} exceeds the {D} features")
        if int(t.shape[0]) and not bool(torch.isfinite(t).all().item()):
            raise ValueError("x holds non-finite values")
        n = int(comm.sum(int(t.shape[0]))[0])
        if n < 2:
            raise ValueError(f"x has {n} rows: a variance needs at least 2")
        # the float64 mean: sums about 0, then about the fp32-rounded mean, whose rounding the first moment takes out
        s0 = comm.sum(k.col_moments64(t)[0])
        c32 = (s0 / n).astype(np.float32)
        s, q = (comm.sum(v) for v in k.col_moments64(t, c32))
        mean = c32.astype(np.float64) + s / n
        sd = np.sqrt(np.maximum((q - s * s / n) / (n - 1), 0.0))
        constant = sd == 0.0
        scale = None
        if self.standardize:
            with np.errstate(divide="ignore"):
                scale = np.where(constant, 0.0, 1.0 / np.where(constant, 1.0, sd))

        V = self.initial_basis(D)
        l = V.shape[1]
        total, lam, S, res = 0.0, None, None, None
        converged, it = False, 0
        while True:
            z, n2 = k.pca_project(t, mean, scale, V, norm2=(it == 0))
            if it == 0:
                total = float(comm.sum(float(n2.sum().item()) if int(t.shape[0]) else 0.0)[0])
            W = comm.sum_tensor(k.pca_backproject(t, mean, scale, z)).cpu().numpy()
            it += 1
            T = V.T @ W
            lam, S = np.linalg.eigh(0.5 * (T + T.T))
            order = np.argsort(-lam, kind="stable")
            lam, S = lam[order], S[:, order]
            VS = V @ S
            top = float(lam[0])
            res = np.linalg.norm(W @ S - VS * lam, axis=0) / top if top > 0.0 else np.zeros(l)
            if float(res[:k_want].max()) <= self.tol:
                converged = True
                break
            if it >= self.max_iter:
                break
            V = np.linalg.qr(W)[0]
        lam_k = np.maximum(lam[:k_want], 0.0)
        self.mean_, self.scale_ = mean, scale
        self.components_ = svd_flip_rows(VS[:, :k_want].T)
        self.explained_variance_ = lam_k / (n - 1)
        self.total_variance_ = total / (n - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.explained_variance_ratio_ = self.explained_variance_ / self.total_variance_
        self.singular_values_ = np.sqrt(lam_k)
        self.n_samples_, self.n_iter_, self.converged_ = n, it, converged
        self.max_residual_ = float(res[:k_want].max())
        self.constant_features_ = int(constant.sum())
        return self

    # -- projections ----------------------------------------------------------------------------------------------------------------
    def project(self, x, kernels=None):
        """(Z, norm2) float64 tensors where the kernels run: the scores [rows, k] of the rows of ``x`` on ``components_`` about
        ``mean_`` (in units of ``scale_``), and the squared norms of the centred rows.  No rounding to fp32."""
        if self.mean_ is None:
            raise RuntimeError("fit first")
        t, k = _cohort(x, kernels)
        if int(t.shape[1]) != self.mean_.shape[0]:
            raise ValueError(f"x has {int(t.shape[1])} features, the fit had {self.mean_.shape[0]}")
        return k.pca_project(t, self.mean_, self.scale_, np.ascontiguousarray(self.components_.T), norm2=True)

    def transform(self, x, residual: bool = False, kernels=None):
        """The scores of the rows of ``x``: an fp32 tensor [rows, k] on the device of the kernels.  ``residual=True`` also returns
        resid2 = max(norm2 - sum_j z_j^2, 0), float64 [rows]: the squared distance of the centred row from the fitted subspace."""
        z, n2 = self.project(x, kernels)
        scores = z.to(torch.float32)
        if not residual:
            return scores
        return scores, (n2 - (z * z).sum(1)).clamp_(min=0.0)

    def fit_transform(self, x, residual: bool = False, comm: Optional[ShardComm] = None, kernels=None):
        return self.fit(x, comm=comm, kernels=kernels).transform(x, residual=residual, kernels=kernels)

    # -- checkpoints ----------------------------------------------------------------------------------------------------------------
    def state(self) -> Dict[str, object]:
        """Plain tensors and numbers: survives ``torch.save`` / ``torch.load(weights_only=True)``."""
        if self.mean_ is None:
            raise RuntimeError("fit first")
        out: Dict[str, object] = {name: getattr(self, name) for name in _PARAMS}
        for name in _ARRAYS:
            v = getattr(self, name)
            out[name] = None if v is None else torch.from_numpy(np.array(v, dtype=np.float64, copy=True))
        for name in _NUMBERS:
            v = getattr(self, name)
            out[name] = bool(v) if isinstance(v, (bool, np.bool_)) else int(v) if isinstance(v, (int, np.integer)) else float(v)
        return out

    @classmethod
    def from_state(cls, state: Dict[str, object]) -> "DevicePCA":
        self = cls(**{name: state[name] for name in _PARAMS})
        for name in _ARRAYS:
            v = state[name]
            setattr(self, name, None if v is None else v.detach().cpu().numpy().astype(np.float64))
        for name in _NUMBERS:
            setattr(self, name, state[name])
        return self


def embedding_rows(comm: ShardComm, kernels, x: torch.Tensor, y: torch.Tensor, n_components: int = 10, standardize: bool = False,
                   **pca_options) -> Dict[str, object]:
    """What ``embedding_summary`` reads, from the real cohort ``x`` and the synthetic cohort ``y`` (float32 [rows, D] tensors;
    ``y`` is this rank's row shard when ``comm`` is active, ``x`` is replicated).  One ``DevicePCA`` is fitted on each cohort (the
    synthetic one through ``comm``), both cohorts are projected onto the REAL components about the real mean, the synthetic scores'
    float64 sums are added over the ranks, the fp32 scores and the residuals are gathered (``gather_rows``), and one
    ``kernels.marginals`` call on the two [rows, k] score matrices gives the KS extremes and the Wasserstein-1 distance of every
    component."""
    one = ShardComm(False)                     # the replicated real cohort never communicates
    real = DevicePCA(n_components, standardize=standardize, **pca_options).fit(x, comm=one, kernels=kernels)
    synth = DevicePCA(n_components, standardize=standardize, **pca_options).fit(y, comm=comm, kernels=kernels)
    zr, n2r = real.project(x, kernels)
    zs, n2s = real.project(y, kernels)
    rr = (n2r - (zr * zr).sum(1)).clamp_(min=0.0)
    rs = (n2s - (zs * zs).sum(1)).clamp_(min=0.0)
    k = real.components_.shape[0]
    sums = np.concatenate([zs.sum(0).cpu().numpy(), (zs * zs).sum(0).cpu().numpy(), [float(n2s.sum().item())]]) if int(y.shape[0]) \
        else np.zeros(2 * k + 1)
    sums = comm.sum(sums)
    real_scores = zr.to(torch.float32).contiguous()
    synth_scores = comm.gather_rows(zs.to(torch.float32).contiguous())
    synth_resid = comm.gather_rows(rs.contiguous())
    marg = kernels.marginals(real_scores, synth_scores)
    return {"real": real, "synth": synth, "n_real": int(x.shape[0]), "n_synth": int(synth_scores.shape[0]),
            "synth_score_sum": sums[:k], "synth_score_sumsq": sums[k:2 * k], "synth_norm2_sum": float(sums[2 * k]),
            "ks_dmax": np.asarray(marg["ks_dmax"], dtype=np.int64), "ks_dmin": np.asarray(marg["ks_dmin"], dtype=np.int64),
            "w1": np.asarray(marg["w1"], dtype=np.float64),
            "real_scores": real_scores, "synth_scores": synth_scores,
            "real_resid2": rr.cpu().numpy().astype(np.float64), "synth_resid2": synth_resid.cpu().numpy().astype(np.float64)}


def embedding_summary(rows: Dict[str, object], quantile: float = 0.99) -> Dict[str, float]:
    """The ``pca_*`` figures from ``embedding_rows`` (pure NumPy, float64).  With lambda_i the real eigenvalues
    (``explained_variance_``), z the synthetic scores on the real components about the real mean, m synthetic rows:

      ``pca_components``, ``pca_converged``, ``pca_iterations_real`` / ``_synth``, ``pca_constant_features``     the two fits
      ``pca_explained_share_real``        the real cohort's variance inside its own k components
      ``pca_captured_share_synth``        sum z^2 / sum |u|^2 over the synthetic rows: their share inside the REAL subspace
      ``pca_variance_ratio_<i>``          i = 1 .. k: the sample variance of z_i over lambda_i -- below 1: the axis is flattened;
                                          ``_mean``, ``_min``, ``_max`` over the components
      ``pca_mean_shift_max``              max_i |mean z_i| / sqrt(lambda_i)
      ``pca_wasserstein_distance_mean``   the reference's figure: the mean over the components of the W1 of the scores, unscaled
      ``pca_w1_scaled_mean`` / ``_max`` / ``_max_component``    W1 over sqrt(lambda_i); the component (1-based) of the maximum
      ``pca_ks_mean`` / ``_max``          the two-sample KS distance of the scores
      ``pca_residual_ratio``              the mean synthetic resid2 over the mean real resid2
      ``pca_offmanifold_share``           the share of synthetic rows whose resid2 exceeds the ``quantile``-quantile
                                          (``numpy.quantile``'s default) of the real rows' resid2
      ``pca_subspace_cos_min`` / ``_mean``     the singular values of components_real @ components_synth^T: the cosines of the
                                          principal angles between the two fitted subspaces"""
    if not 0.0 <= float(quantile) <= 1.0:
        raise ValueError("quantile must lie in [0, 1]")
    real, synth = rows["real"], rows["synth"]
    lam = np.asarray(real.explained_variance_, dtype=np.float64)
    k, n, m = lam.shape[0], int(rows["n_real"]), int(rows["n_synth"])
    if m < 2:
        raise ValueError(f"synthetic has {m} rows: a variance needs at least 2")
    s1, s2 = np.asarray(rows["synth_score_sum"], dtype=np.float64), np.asarray(rows["synth_score_sumsq"], dtype=np.float64)
    var = np.maximum(s2 - s1 * s1 / m, 0.0) / (m - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(lam > 0, var / lam, np.nan)
        shift = np.where(lam > 0, np.abs(s1 / m) / np.sqrt(lam), np.nan)
        w1s = np.where(lam > 0, np.asarray(rows["w1"], dtype=np.float64) / np.sqrt(lam), np.nan)
        captured = float(s2.sum() / rows["synth_norm2_sum"]) if rows["synth_norm2_sum"] > 0 else float("nan")
    dmax, dmin = np.asarray(rows["ks_dmax"], dtype=np.int64), np.asarray(rows["ks_dmin"], dtype=np.int64)
    ks = np.maximum(np.maximum(dmax, -dmin), 0).astype(np.float64) / (float(n) * float(m))
    rr, rs = np.asarray(rows["real_resid2"], dtype=np.float64), np.asarray(rows["synth_resid2"], dtype=np.float64)
    cos = np.linalg.svd(real.components_ @ synth.components_.T, compute_uv=False)

    def over(v, fn):
        return float(fn(v)) if np.isfinite(v).any() else float("nan")

    out: Dict[str, float] = {"pca_components": k, "pca_converged": bool(real.converged_ and synth.converged_),
                             "pca_iterations_real": int(real.n_iter_), "pca_iterations_synth": int(synth.n_iter_),
                             "pca_constant_features": int(real.constant_features_),
                             "pca_explained_share_real": float(np.sum(real.explained_variance_ratio_)),
                             "pca_captured_share_synth": captured}
    for i in range(k):
        out[f"pca_variance_ratio_{i + 1}"] = float(ratio[i])
    out["pca_variance_ratio_mean"] = over(ratio, np.nanmean)
    out["pca_variance_ratio_min"] = over(ratio, np.nanmin)
    out["pca_variance_ratio_max"] = over(ratio, np.nanmax)
    out["pca_mean_shift_max"] = over(shift, np.nanmax)
    out["pca_wasserstein_distance_mean"] = float(np.mean(rows["w1"]))
    out["pca_w1_scaled_mean"] = over(w1s, np.nanmean)
    out["pca_w1_scaled_max"] = over(w1s, np.nanmax)
    out["pca_w1_scaled_max_component"] = int(np.nanargmax(w1s)) + 1 if np.isfinite(w1s).any() else 0
    out["pca_ks_mean"] = float(ks.mean())
    out["pca_ks_max"] = float(ks.max())
    with np.errstate(divide="ignore", invalid="ignore"):
        out["pca_residual_ratio"] = float(rs.mean() / rr.mean())
    out["pca_offmanifold_share"] = float((rs > np.quantile(rr, float(quantile))).mean())
    out["pca_subspace_cos_min"] = float(cos.min())
    out["pca_subspace_cos_mean"] = float(cos.mean())
    return out
