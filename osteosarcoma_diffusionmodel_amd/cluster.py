"""Subtype structure: Lloyd's k-means over a device-resident cohort and the subtype-fidelity figures built on it (DESIGN.md section
3.25).  The two halves of an iteration are two library calls -- ``kernels.nearest`` (``osd_val_nearest``: every row against the K
centroids in one Gram pass, ties to the smallest index, distances recomputed exactly) and ``kernels.label_sums``
(``osd_val_label_sums``: per-label column sums in double, bit-reproducible) -- and everything else here is host logic over their
results: ``kernels`` is any object with those two methods (``validation.DeviceKernels``, or a float64 NumPy stand-in in the CPU
tests), the way ``utility.fit_glm`` is driven.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .parallel import ShardComm

MAX_CLUSTERS = 64                 # K of one osd_val_label_sums call


@dataclass
class KMeansResult:
    centroids: torch.Tensor       # float32 [K, D], on x's device
    labels: torch.Tensor          # int32 [N]: the nearest centroid of every row
    d2: torch.Tensor              # float32 [N]: its squared distance, recomputed directly
    counts: np.ndarray            # int64 [K]
    inertia: float                # float64 sum of d2
    iterations: int               # assignment passes
    converged: bool               # the last pass changed no label
    empty: List[int]              # clusters without a row: they kept their centroid


def _check(x: torch.Tensor, n_clusters: int) -> int:
    K = int(n_clusters)
    if not 1 <= K <= MAX_CLUSTERS:
        raise ValueError(f"n_clusters must lie in [1, {MAX_CLUSTERS}], got {K}")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be a [rows, features] tensor")
    if x.shape[0] < K:
        raise ValueError(f"x has {x.shape[0]} rows: {K} clusters need at least as many")
    return K


def kmeans_pp_indices(x: torch.Tensor, K: int, rng: np.random.Generator, kernels) -> List[int]:
    """Row numbers of k-means++ centres: the first is ``rng.integers(N)``, each further one is drawn proportionally to the float64
    cast of the recomputed squared distance to the nearest centre chosen so far (``np.searchsorted(cumsum, rng.random() * total,
    side="right")``, clipped), and the smallest unchosen row where that total is 0 (fewer distinct rows than centres)."""
    N = int(x.shape[0])
    chosen = [int(rng.integers(N))]
    while len(chosen) < K:
        centres = x.index_select(0, torch.as_tensor(chosen, dtype=torch.int64, device=x.device)).contiguous()
        d2, _ = kernels.nearest(x, centres)
        cum = np.cumsum(d2.detach().cpu().numpy().astype(np.float64))
        total = float(cum[-1])
        if total > 0.0:
            i = min(int(np.searchsorted(cum, rng.random() * total, side="right")), N - 1)
        else:
            taken = set(chosen)
            i = next(j for j in range(N) if j not in taken)
        chosen.append(i)
    return chosen


def lloyd(x: torch.Tensor, centroids: torch.Tensor, max_iter: int, kernels) -> KMeansResult:
    """Lloyd iterations from ``centroids`` (float32 [K, D] on x's device).  A pass assigns every row; when no label differs from the
    previous pass the fit has converged.  Otherwise C_k = float32(sums_k / counts_k) in double from ``kernels.label_sums``; an empty
    cluster keeps its centroid.  At most ``max_iter`` assignment passes: the centroids returned are the ones the returned labels and
    distances were taken against."""
    K = int(centroids.shape[0])
    C = centroids.to(device=x.device, dtype=torch.float32).contiguous()
    prev, converged, iterations = None, False, 0
    while True:
        d2, labels = kernels.nearest(x, C)
        iterations += 1
        if prev is not None and torch.equal(labels, prev):
            converged = True
            break
        if iterations >= max_iter:
            break
        sums, counts, _ = kernels.label_sums(x, labels, K)
        filled = counts > 0
        mean = (sums / counts.clamp(min=1).to(torch.float64).unsqueeze(1)).to(torch.float32)
        C = torch.where(filled.unsqueeze(1), mean, C).contiguous()
        prev = labels
    counts = torch.bincount(labels.to(torch.int64), minlength=K).cpu().numpy().astype(np.int64)
    return KMeansResult(centroids=C, labels=labels, d2=d2, counts=counts, inertia=float(d2.to(torch.float64).sum().item()),
                        iterations=iterations, converged=converged, empty=[int(k) for k in np.flatnonzero(counts == 0)])


def kmeans(x: torch.Tensor, n_clusters: int, *, init="k-means++", seed: int = 0, n_init: int = 1, max_iter: int = 100,
           kernels=None) -> KMeansResult:
    """Lloyd's k-means of the rows of ``x`` (float32 [N, D], finite, N >= K, 1 <= K <= 64; Euclidean distances over the columns as
    given).  ``init``: "k-means++" (restart r draws from ``np.random.default_rng(seed + r)``; ``kmeans_pp_indices``) or an explicit
    [K, D] array, used as given.  ``n_init`` restarts keep the lowest inertia, ties to the earliest.  ``kernels``: an object with
    ``nearest`` and ``label_sums`` (default: ``validation.DeviceKernels`` on x's device)."""
    K = _check(x, n_clusters)
    max_iter, n_init = int(max_iter), int(n_init)
    if max_iter < 1 or n_init < 1:
        raise ValueError("max_iter and n_init must be at least 1")
    if kernels is None:
        from .validation import DeviceKernels
        kernels = DeviceKernels(x.device)
    explicit = not isinstance(init, str)
    if explicit:
        c0 = init if isinstance(init, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32))
        if tuple(c0.shape) != (K, int(x.shape[1])):
            raise ValueError(f"init must be [{K}, {int(x.shape[1])}], got {tuple(c0.shape)}")
    elif init != "k-means++":
        raise ValueError("init must be 'k-means++' or a [K, D] array")
    best: Optional[KMeansResult] = None
    for restart in range(1 if explicit else n_init):
        if not explicit:
            rows = kmeans_pp_indices(x, K, np.random.default_rng(int(seed) + restart), kernels)
            c0 = x.index_select(0, torch.as_tensor(rows, dtype=torch.int64, device=x.device))
        fit = lloyd(x, c0, max_iter, kernels)
        if best is None or fit.inertia < best.inertia:
            best = fit
    return best


def renumber_order(counts) -> np.ndarray:
    """order[new] = old: clusters by descending count, ties by ascending index."""
    return np.argsort(-np.asarray(counts, dtype=np.int64), kind="stable")


def _label_stats(comm, kernels, t: torch.Tensor, labels, K: int, value, cond):
    """(counts int64 [K], value sums float64 [K], label sums float64 [K, D] on t's device, condition sums float64 [K, C] or None) of
    one cohort, summed over ``comm``; a shard without rows contributes zeros."""
    D = int(t.shape[1])
    if int(t.shape[0]):
        sums, counts, vs = kernels.label_sums(t, labels, K, value=value)
        counts, vs = counts.cpu().numpy().astype(np.int64), vs.cpu().numpy().astype(np.float64)
    else:
        sums = torch.zeros((K, D), dtype=torch.float64, device=t.device)
        counts, vs = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.float64)
    counts = comm.sum(counts).astype(np.int64)
    vs = comm.sum(vs)
    sums = comm.sum_tensor(sums)
    cs = None
    if cond is not None:
        if int(t.shape[0]):
            cs = kernels.label_sums(cond, labels, K)[0].cpu().numpy().astype(np.float64)
        else:
            cs = np.zeros((K, int(cond.shape[1])), dtype=np.float64)
        cs = comm.sum(cs.ravel()).reshape(K, -1)
    return counts, vs, sums, cs


def subtype_rows(comm, kernels, x: torch.Tensor, y: torch.Tensor, n_clusters: int, *, conditions=None, names=None, seed: int = 0,
                 n_init: int = 4, max_iter: int = 100) -> Dict[str, object]:
    """The sums ``subtype_summary`` reads, from the real cohort ``x`` and the synthetic cohort ``y`` (float32 [rows, D] tensors on one
    device; ``y`` is this rank's row shard when ``comm`` is active, ``x`` is replicated).  The fp32 column means of ``x`` are
    subtracted from working copies of both (translation changes no cluster and keeps the Gram pass's expanded distance out of
    cancellation), k-means is fitted on ``x``, the clusters are renumbered by descending real count, every row of ``y`` goes to its
    nearest centroid, and one ``label_sums`` per cohort with value = d2 gives counts, sums of squared distances and label sums.
    ``conditions``: (real, synthetic) float32 [rows, C] tensors, one more ``label_sums`` each.  Also returned: the centroids
    (original coordinates, float64), both label arrays and both d2 arrays (the synthetic ones are the shard's)."""
    K = _check(x, n_clusters)
    N, D = int(x.shape[0]), int(x.shape[1])
    whole = torch.zeros(N, dtype=torch.int32, device=x.device)
    center = (kernels.label_sums(x, whole, 1)[0][0] / float(N)).to(torch.float32)       # the column means: label sums with one label
    xc, yc = (x - center).contiguous(), (y - center).contiguous()
    fit = kmeans(xc, K, seed=seed, n_init=n_init, max_iter=max_iter, kernels=kernels)
    order = renumber_order(fit.counts)
    new_of_old = np.empty(K, dtype=np.int32)
    new_of_old[order] = np.arange(K, dtype=np.int32)
    C = fit.centroids.index_select(0, torch.as_tensor(order, dtype=torch.int64, device=x.device)).contiguous()
    real_labels = torch.as_tensor(new_of_old, device=x.device)[fit.labels.to(torch.int64)].contiguous()
    if int(yc.shape[0]):
        synth_d2, synth_labels = kernels.nearest(yc, C)
    else:
        synth_d2 = torch.empty(0, dtype=torch.float32, device=x.device)
        synth_labels = torch.empty(0, dtype=torch.int32, device=x.device)
    rc, sc = (None, None) if conditions is None else conditions
    one = ShardComm(False)                     # the replicated real cohort never communicates
    n, rd2, _, rcs = _label_stats(one, kernels, xc, real_labels, K, fit.d2, rc)
    m, sd2, ssums, scs = _label_stats(comm, kernels, yc, synth_labels, K, synth_d2, sc)
    Cd = C.to(torch.float64)
    rows = {"k": K, "inertia": fit.inertia, "iterations": fit.iterations, "converged": fit.converged,
            "real_counts": n, "synth_counts": m, "real_d2_sums": rd2, "synth_d2_sums": sd2,
            "centroids_centered": Cd.cpu().numpy(), "synth_sums": ssums.cpu().numpy(),
            "centroids": (Cd + center.to(torch.float64)).cpu().numpy(),
            "real_labels": real_labels.cpu().numpy(), "synth_labels": synth_labels.cpu().numpy(),
            "real_d2": fit.d2.cpu().numpy(), "synth_d2": synth_d2.cpu().numpy()}
    if conditions is not None:
        rows["condition_names"] = [str(v) for v in names]
        rows["real_condition_sums"], rows["synth_condition_sums"] = rcs, scs
    return rows


def subtype_summary(rows: Dict[str, object]) -> Dict[str, float]:
    """The ``subtype_*`` figures from the per-subtype sums of ``subtype_rows`` (pure NumPy, float64).  With n_k / m_k the real /
    synthetic counts of subtype k, p = n / N and q = m / M:

      ``subtype_k``, ``subtype_inertia``, ``subtype_iterations``, ``subtype_converged``   the fit on the real cohort
      ``subtype_real_share_<k>``, ``subtype_synth_share_<k>``     p_k, q_k
      ``subtype_js_divergence``, ``subtype_tv_distance``          Jensen-Shannon divergence, base 2, in [0, 1]; sum |p - q| / 2
      ``subtype_missing``, ``subtype_min_share_ratio``            #{k : n_k > 0, m_k = 0}; min over n_k > 0 of q_k / p_k
      ``subtype_dispersion_ratio_<k>``, ``..._min``               (sum of d2 over the synthetic rows of k / m_k) / (the same over the
                                                                  real rows); NaN where either side is empty or the real dispersion
                                                                  is 0; the minimum over the finite ones
      ``subtype_centroid_shift_<k>``, ``..._max``                 |mean of the synthetic rows of k - centroid k| / sqrt(real mean d2)
      ``subtype_condition_gap_<name>``                            max over the subtypes both cohorts populate of |mean of the
                                                                  condition among the real rows of k - among the synthetic rows|

    ``real_counts`` / ``synth_counts`` [K], ``real_d2_sums`` / ``synth_d2_sums`` [K], ``centroids_centered`` and ``synth_sums`` [K, D]
    (one coordinate system), and optionally ``condition_names`` with ``real_condition_sums`` / ``synth_condition_sums`` [K, C]."""
    n = np.asarray(rows["real_counts"], dtype=np.int64)
    m = np.asarray(rows["synth_counts"], dtype=np.int64)
    K = n.shape[0]
    if m.shape != (K,) or K < 1:
        raise ValueError("real_counts and synth_counts must hold one count per subtype")
    N, M = int(n.sum()), int(m.sum())
    if N < 1 or M < 1:
        raise ValueError("a subtype summary needs at least one row in each cohort")
    nan = float("nan")
    nf, mf = n.astype(np.float64), m.astype(np.float64)
    p, q = nf / N, mf / M
    mix = 0.5 * (p + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        # counts times logs, divided once: disjoint supports give exactly 1, identical shares exactly 0
        js = 0.5 * float(np.where(n > 0, nf * np.log2(p / mix), 0.0).sum()) / N + 0.5 * float(np.where(m > 0, mf * np.log2(q / mix), 0.0).sum()) / M
        ratio = np.where(n > 0, q / p, np.inf)
        rdisp = np.where(n > 0, np.asarray(rows["real_d2_sums"], dtype=np.float64) / nf, nan)
        sdisp = np.where(m > 0, np.asarray(rows["synth_d2_sums"], dtype=np.float64) / mf, nan)
        live = (n > 0) & (m > 0) & (rdisp > 0)
        disp = np.where(live, sdisp / rdisp, nan)
        mean = np.asarray(rows["synth_sums"], dtype=np.float64) / mf[:, None]
        shift = np.where(live, np.sqrt(((mean - np.asarray(rows["centroids_centered"], dtype=np.float64)) ** 2).sum(1)) / np.sqrt(rdisp), nan)
    out: Dict[str, float] = {"subtype_k": K, "subtype_inertia": float(rows["inertia"]), "subtype_iterations": int(rows["iterations"]),
                             "subtype_converged": bool(rows["converged"])}
    for k in range(K):
        out[f"subtype_real_share_{k}"] = float(p[k])
        out[f"subtype_synth_share_{k}"] = float(q[k])
    out["subtype_js_divergence"] = min(max(js, 0.0), 1.0)
    out["subtype_tv_distance"] = 0.5 * float(np.abs(p - q).sum())
    out["subtype_missing"] = int(((n > 0) & (m == 0)).sum())
    out["subtype_min_share_ratio"] = float(ratio.min())
    for k in range(K):
        out[f"subtype_dispersion_ratio_{k}"] = float(disp[k])
    out["subtype_dispersion_ratio_min"] = float(np.nanmin(disp)) if np.isfinite(disp).any() else nan
    for k in range(K):
        out[f"subtype_centroid_shift_{k}"] = float(shift[k])
    out["subtype_centroid_shift_max"] = float(np.nanmax(shift)) if np.isfinite(shift).any() else nan
    if "condition_names" in rows:
        both = (n > 0) & (m > 0)
        rc = np.asarray(rows["real_condition_sums"], dtype=np.float64)
        sc = np.asarray(rows["synth_condition_sums"], dtype=np.float64)
        for j, name in enumerate(rows["condition_names"]):
            with np.errstate(divide="ignore", invalid="ignore"):
                gap = np.abs(rc[:, j] / nf - sc[:, j] / mf)
            out[f"subtype_condition_gap_{name}"] = float(gap[both].max()) if both.any() else nan
    return out
