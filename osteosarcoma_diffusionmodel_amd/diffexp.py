"""Differential-signal fidelity: do the features that separate two groups of patients in the real cohort --
metastatic against non-metastatic, say -- separate them in the synthetic cohort too, in the same direction and by the same amount?

Everything that scales with the number of patients is one ``DeviceKernels.group_ranks`` call per cohort and contrast
(``osd_val_group_ranks``: per feature twice the Mann-Whitney U, the tie correction and each group's centred moments); this module is
the float64 host code over those D-vectors: ``group_statistics`` (AUC, rank-biserial effect, the normal approximation's z and p,
Benjamini-Hochberg q, mean difference, Welch t, Cohen's d), ``contrast_labels`` (a condition column as case / control labels),
``contrast_summary`` (the synthetic cohort's per-feature figures against the real one's) and ``differential_metrics`` (all contrasts).
The kernels object is an argument, so the CPU tests drive the same code over a NumPy stand-in."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

STAT_FIELDS = ("auc", "effect", "z", "p", "q", "mean_diff", "welch_t", "cohen_d")
MEAN_KEYS = ("effect_pearson", "effect_spearman", "effect_slope", "sign_agreement", "precision", "recall", "topk_jaccard",
             "false_signal_share", "max_abs_effect_gap")


def bh_qvalues(p) -> np.ndarray:
    """Benjamini-Hochberg q-values of the p-values p [m]: with p_(1) <= ... <= p_(m), q_(i) = min_{j >= i} p_(j) m / j, at most 1, back in
    p's order (a stable sort: equal p-values get equal q-values whatever their order)."""
    p = np.asarray(p, dtype=np.float64)
    m = p.shape[0]
    order = np.argsort(p, kind="stable")
    scaled = p[order] * m / np.arange(1, m + 1, dtype=np.float64)
    q = np.empty(m, dtype=np.float64)
    q[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return q


def group_statistics(rows: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The per-feature figures (float64 [D] each, ``STAT_FIELDS``) from the arrays of ``DeviceKernels.group_ranks``, cases against
    controls.  With U = u2 / 2, N = na + nb:

      ``auc``        U / (na nb): the chance that a case's value exceeds a control's, ties counted 1/2
      ``effect``     the rank-biserial correlation 2 AUC - 1, in [-1, 1]
      ``z``, ``p``   (U - na nb / 2) / sqrt(na nb / 12 ((N + 1) - ties / (N (N - 1)))) and its two-sided normal p-value: what
                     ``scipy.stats.mannwhitneyu(method="asymptotic", use_continuity=False)`` returns
      ``q``          ``bh_qvalues`` of p over the D features
      ``mean_diff``  mean of the cases - mean of the controls (the centre cancels)
      ``welch_t``    mean_diff / sqrt(var_a / na + var_b / nb), variances with ddof = 1
      ``cohen_d``    mean_diff / the pooled standard deviation

    A feature that is constant over the pooled rows has ties = N^3 - N, hence no variance: it gets effect 0, z 0, p 1 and q 1, and 0
    for the two moment ratios (0 / 0); a non-zero difference over a zero spread keeps its infinity."""
    na, nb = float(rows["na"]), float(rows["nb"])
    if na < 1 or nb < 1:
        raise ValueError("both groups need at least one row")
    n = na + nb
    u2 = np.asarray(rows["u2"], dtype=np.int64).astype(np.float64)
    ties = np.asarray(rows["ties"], dtype=np.int64).astype(np.float64)
    s, q = np.asarray(rows["sum"], dtype=np.float64), np.asarray(rows["sumsq"], dtype=np.float64)
    from scipy.special import ndtr
    u = u2 / 2.0
    auc = u / (na * nb)
    var = na * nb / 12.0 * ((n + 1.0) - ties / (n * (n - 1.0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(var > 0, (u - na * nb / 2.0) / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)
        p = np.minimum(2.0 * ndtr(-np.abs(z)), 1.0)
        mean = [s[g] / cnt for g, cnt in ((0, na), (1, nb))]
        v = [np.maximum(q[g] - s[g] * s[g] / cnt, 0.0) / (cnt - 1.0) if cnt > 1 else np.zeros_like(s[g]) for g, cnt in ((0, na), (1, nb))]
        diff = mean[0] - mean[1]
        welch = diff / np.sqrt(v[0] / na + v[1] / nb)
        pooled = np.sqrt(((na - 1.0) * v[0] + (nb - 1.0) * v[1]) / (n - 2.0)) if n > 2 else np.zeros_like(diff)
        cohen = diff / pooled
    welch[np.isnan(welch)] = 0.0
    cohen[np.isnan(cohen)] = 0.0
    return {"auc": auc, "effect": 2.0 * auc - 1.0, "z": z, "p": p, "q": bh_qvalues(p), "mean_diff": diff, "welch_t": welch,
            "cohen_d": cohen}


def contrast_labels(real_col, synth_col):
    """(real labels, synthetic labels, threshold): a condition column of both cohorts as int32 case (1) / control (0) labels.  A
    column whose values all lie in {0, 1} in BOTH cohorts is used as it is (threshold None); any other column is split at the REAL
    cohort's median -- a case is a value above it -- and the same threshold is applied to the synthetic cohort."""
    r, s = np.asarray(real_col, dtype=np.float64).ravel(), np.asarray(synth_col, dtype=np.float64).ravel()
    if np.isin(r, (0.0, 1.0)).all() and np.isin(s, (0.0, 1.0)).all():
        return r.astype(np.int32), s.astype(np.int32), None
    thr = float(np.median(r))
    return (r > thr).astype(np.int32), (s > thr).astype(np.int32), thr


def cohort_statistics(k, x: torch.Tensor, labels: np.ndarray) -> Dict[str, np.ndarray]:
    """``group_statistics`` of one cohort and contrast: the moments are centred at the fp32-rounded column means of the whole cohort
    (``k.col_centered_moments`` about 0), so that the variances lose nothing to cancellation; the kernel's arrays ride along."""
    n = int(x.shape[0])
    s0, _ = k.col_centered_moments(x)
    center = (np.asarray(s0, dtype=np.float64) / n).astype(np.float32)
    rows = k.group_ranks(x, torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)), center)
    out = group_statistics(rows)
    out.update({name: rows[name] for name in ("u2", "ties", "na", "nb")})
    return out


def _pearson(a: np.ndarray, b: np.ndarray) -> float:
    a, b = a - a.mean(), b - b.mean()
    den = float(np.sqrt((a * a).sum() * (b * b).sum()))
    return float((a * b).sum() / den) if den > 0 else float("nan")


def _share(mask: np.ndarray) -> float:
    return float(mask.mean()) if mask.size else float("nan")


def contrast_summary(real: Dict[str, np.ndarray], synth: Dict[str, np.ndarray], alpha: float = 0.05, top_k: int = 50,
                     bounds: Optional[Sequence[int]] = None, names: Optional[Sequence[str]] = None) -> Dict[str, float]:
    """One contrast's figures from the two cohorts' ``group_statistics``; a hit is a feature with q < alpha:

      ``effect_pearson``, ``effect_spearman``  over the features, of the synthetic against the real rank-biserial effects
      ``effect_slope``         the least-squares slope (with intercept) of synthetic on real: below 1 flattened, above 1 exaggerated
      ``sign_agreement``       over the real hits, the share whose synthetic effect has the real effect's sign
      ``real_hits``, ``synth_hits``, ``precision``, ``recall``  of the synthetic hits against the real ones
      ``topk_jaccard``         of the ``top_k`` features by |effect| in either cohort (all D when D < top_k)
      ``false_signal_share``   the share of synthetic hits among the features with real q > 0.5
      ``max_abs_effect_gap``, ``max_gap_feature``  the largest |synthetic - real effect| and its column index
      with more than one block, ``effect_pearson_<block>``

    A share over an empty set and a correlation of a constant vector are NaN."""
    er, es = np.asarray(real["effect"], dtype=np.float64), np.asarray(synth["effect"], dtype=np.float64)
    qr, qs = np.asarray(real["q"], dtype=np.float64), np.asarray(synth["q"], dtype=np.float64)
    D = er.shape[0]
    if es.shape != (D,) or qr.shape != (D,) or qs.shape != (D,) or D < 1:
        raise ValueError("one entry per feature in every array")
    from scipy.stats import rankdata
    hr, hs = qr < alpha, qs < alpha
    cr = er - er.mean()
    var = float((cr * cr).sum())
    kk = max(1, min(int(top_k), D))
    top_r, top_s = (set(np.argsort(-np.abs(e), kind="stable")[:kk].tolist()) for e in (er, es))
    gap = np.abs(es - er)
    out = {
        "effect_pearson": _pearson(er, es),
        "effect_spearman": _pearson(rankdata(er), rankdata(es)),
        "effect_slope": float((cr * (es - es.mean())).sum() / var) if var > 0 else float("nan"),
        "sign_agreement": _share(np.sign(es[hr]) == np.sign(er[hr])),
        "real_hits": int(hr.sum()),
        "synth_hits": int(hs.sum()),
        "precision": _share(hr[hs]),
        "recall": _share(hs[hr]),
        "topk_jaccard": len(top_r & top_s) / float(len(top_r | top_s)),
        "false_signal_share": _share(hs[qr > 0.5]),
        "max_abs_effect_gap": float(gap.max()),
        "max_gap_feature": int(np.argmax(gap)),
    }
    if bounds is not None and len(bounds) > 2:
        for name, lo, hi in zip(names, bounds, bounds[1:]):
            out[f"effect_pearson_{name}"] = _pearson(er[lo:hi], es[lo:hi])
    return out


def differential_metrics(k, x: torch.Tensor, real_cond: np.ndarray, y: torch.Tensor, synth_cond: np.ndarray, names: Sequence[str],
                         bounds: Optional[Sequence[int]] = None, block_names: Optional[Sequence[str]] = None, alpha: float = 0.05,
                         top_k: int = 50):
    """(summary, rows) over every column of the condition matrices [rows, K] (float64, host): per contrast with two non-empty groups
    in both cohorts the keys of ``contrast_summary`` as ``de_<key>_<contrast>``, then ``de_<key>_mean`` over the contrasts for the
    keys of ``MEAN_KEYS`` (NaNs left out), ``de_contrasts`` and ``de_skipped`` -- the contrasts with an empty group in either cohort,
    which add no other key.  ``rows[contrast]`` holds ``real`` and ``synthetic`` (``cohort_statistics``) and ``threshold``."""
    summary: Dict[str, float] = {}
    rows: Dict[str, dict] = {}
    per_key = {key: [] for key in MEAN_KEYS}
    skipped = 0
    for j, name in enumerate(names):
        lr, ls, thr = contrast_labels(real_cond[:, j], synth_cond[:, j])
        if min(int((lr == 1).sum()), int((lr == 0).sum()), int((ls == 1).sum()), int((ls == 0).sum())) < 1:
            skipped += 1
            continue
        real, synth = cohort_statistics(k, x, lr), cohort_statistics(k, y, ls)
        one = contrast_summary(real, synth, alpha, top_k, bounds, block_names)
        summary.update({f"de_{key}_{name}": v for key, v in one.items()})
        for key in MEAN_KEYS:
            per_key[key].append(one[key])
        rows[name] = {"real": real, "synthetic": synth, "threshold": thr}
    for key, vals in per_key.items():
        live = [v for v in vals if not np.isnan(v)]
        if vals:
            summary[f"de_{key}_mean"] = float(np.mean(live)) if live else float("nan")
    summary["de_contrasts"] = len(names) - skipped
    summary["de_skipped"] = skipped
    return summary, rows
