"""Pathway-enrichment fidelity: is a gene set -- the p53 pathway, say -- up or down in the metastatic patients
of the synthetic cohort as it is in the real one?  Preranked gene-set enrichment analysis (Subramanian et al. 2005) with a gene-label
permutation null, per cohort and contrast:

  the ranking statistic is the per-gene Mann-Whitney z of ``diffexp.cohort_statistics``; the genes are ranked by it, descending
  (``rank_positions``), and position i of the list weighs |z at i| ** weight;
  one ``DeviceKernels.gsea`` call (``osd_val_gsea``) gives, for every set, the positive and the negative extreme of the weighted
  running sum under the identity and under P permutations of the gene labels that all sets share;
  this module is the float64 host code over those arrays: ``enrichment_statistics`` (ES, NES, p, Benjamini-Hochberg q, leading-edge
  size), ``enrichment_summary`` (the synthetic cohort's sets against the real one's) and ``enrichment_metrics`` (all contrasts).

The kernels object is an argument, so the CPU tests drive the same code over a NumPy stand-in."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import diffexp as DE

STAT_FIELDS = ("es", "nes", "p", "q", "leading_edge")
MEAN_KEYS = ("nes_pearson", "nes_spearman", "nes_slope", "sign_agreement", "precision", "recall", "false_signal_share",
             "max_abs_nes_gap")
MAX_SET = 1024            # members of a set osd_val_gsea takes


def rank_positions(stat) -> np.ndarray:
    """pos int64 [D]: gene g sits at position pos[g] of the list ranked by ``stat`` descending, equal values by ascending index
    (-0.0 and +0.0 are equal)."""
    stat = np.asarray(stat, dtype=np.float64)
    if stat.ndim != 1 or not np.isfinite(stat).all():
        raise ValueError("the ranking statistic must be a finite vector")
    order = np.argsort(-stat, kind="stable")
    pos = np.empty(stat.shape[0], dtype=np.int64)
    pos[order] = np.arange(stat.shape[0], dtype=np.int64)
    return pos


def position_weights(stat, pos, weight: float = 1.0) -> np.ndarray:
    """w float64 [D]: w[pos[g]] = |stat[g]| ** weight (``weight`` = 0: all ones, the classic Kolmogorov-Smirnov form)."""
    w = np.empty(len(pos), dtype=np.float64)
    w[np.asarray(pos)] = np.abs(np.asarray(stat, dtype=np.float64)) ** float(weight)
    return w


def select_sets(gene_sets, D: int, min_size: int = 5, max_size: int = 500, columns=None) -> Tuple[List[str], List[np.ndarray], int]:
    """(names, sets, skipped) from an ordered ``{name: column indices}`` mapping or a [D, S] 0/1 matrix / DataFrame whose columns name
    the sets (a DataFrame with ``columns`` given -- the names of the D data columns -- is first reindexed to them by its row labels,
    rows of absent genes dropped).  Members are de-duplicated and sorted; a set with fewer than ``min_size`` or more than
    min(``max_size``, 1024, D - 1) members is dropped and counted in ``skipped``."""
    if int(min_size) < 1 or int(max_size) < int(min_size):
        raise ValueError("1 <= min_size <= max_size is needed")
    if hasattr(gene_sets, "items") and not hasattr(gene_sets, "columns"):
        named = [(str(name), np.asarray(list(members), dtype=np.int64).reshape(-1)) for name, members in gene_sets.items()]
    else:
        names = [str(c) for c in gene_sets.columns] if hasattr(gene_sets, "columns") else None
        if columns is not None and hasattr(gene_sets, "reindex"):
            gene_sets = gene_sets.reindex(list(columns)).fillna(0)
        m = np.asarray(gene_sets.values if hasattr(gene_sets, "values") else gene_sets)
        if m.ndim != 2 or m.shape[0] != D:
            raise ValueError(f"a gene-set matrix must be [{D}, sets], got {m.shape}")
        if not np.isin(m, (0, 1)).all():
            raise ValueError("a gene-set matrix holds 0 and 1 only")
        names = names if names is not None else [f"set{s}" for s in range(m.shape[1])]
        named = [(names[s], np.flatnonzero(m[:, s])) for s in range(m.shape[1])]
    hi = min(int(max_size), MAX_SET, D - 1)
    out_names, sets, skipped = [], [], 0
    for name, members in named:
        if members.size and (members.min() < 0 or members.max() >= D):
            raise ValueError(f"set {name!r} holds a column index outside [0, {D})")
        members = np.unique(members)
        if members.size < int(min_size) or members.size > hi:
            skipped += 1
            continue
        out_names.append(name)
        sets.append(members)
    if len(set(out_names)) != len(out_names):
        raise ValueError("the gene sets need distinct names")
    return out_names, sets, skipped


def enrichment_statistics(es_pos, es_neg, lead, sizes) -> Dict[str, np.ndarray]:
    """The per-set figures (``STAT_FIELDS``, [S] each) from the arrays of ``DeviceKernels.gsea`` -- es_pos, es_neg float64 [P + 1, S],
    row 0 observed; lead int [S, 2], the first hit number that attains the observed maximum and minimum; sizes [S]:

      ``es``            per row ES = ES+ if ES+ >= -ES- else ES-; the observed one
      ``nes``           ES / mean |ES_null| over the same-sign nulls -- the permutations with ES_null ES > 0, all of them when ES = 0;
                        NaN when there is none
      ``p``             (1 + #{same-sign nulls with |ES_null| >= |ES|}) / (1 + #same-sign nulls): never 0
      ``q``             ``diffexp.bh_qvalues`` of p over the sets
      ``leading_edge``  the hits up to and including the maximum's when ES > 0, from the minimum's on when ES < 0, 0 when ES = 0

    plus ``same_sign``, the number of same-sign nulls."""
    es_pos, es_neg = np.asarray(es_pos, dtype=np.float64), np.asarray(es_neg, dtype=np.float64)
    lead, sizes = np.asarray(lead, dtype=np.int64), np.asarray(sizes, dtype=np.int64)
    S = sizes.shape[0]
    if es_pos.ndim != 2 or es_pos.shape[1] != S or es_pos.shape[0] < 1 or es_neg.shape != es_pos.shape or lead.shape != (S, 2):
        raise ValueError("es_pos and es_neg must be [permutations + 1, S], lead [S, 2] and sizes [S]")
    es = np.where(es_pos >= -es_neg, es_pos, es_neg)
    obs, null = es[0], es[1:]
    same = (null * obs > 0) | (obs == 0)
    n_same = same.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(same, np.abs(null), 0.0).sum(axis=0) / n_same
        nes = np.where(n_same > 0, obs / scale, np.nan)
    p = (1.0 + (same & (np.abs(null) >= np.abs(obs))).sum(axis=0)) / (1.0 + n_same)
    edge = np.where(obs > 0, lead[:, 0] + 1, np.where(obs < 0, sizes - lead[:, 1], 0))
    return {"es": obs, "nes": nes, "p": p, "q": DE.bh_qvalues(p), "leading_edge": edge.astype(np.int64), "same_sign": n_same.astype(np.int64)}


def enrichment_summary(real: Dict[str, np.ndarray], synth: Dict[str, np.ndarray], alpha: float = 0.05) -> Dict[str, float]:
    """One contrast's figures from the two cohorts' ``enrichment_statistics``; a hit is a set with q < alpha:

      ``nes_pearson``, ``nes_spearman``  over the sets whose NES is a number in both cohorts, synthetic against real
      ``nes_slope``            the least-squares slope (with intercept) of synthetic on real NES over the same sets
      ``sign_agreement``       over the real hits, the share whose synthetic ES has the real ES's sign
      ``real_hits``, ``synth_hits``, ``precision``, ``recall``  of the synthetic hits against the real ones
      ``false_signal_share``   the share of synthetic hits among the sets with real q > 0.5
      ``max_abs_nes_gap``, ``max_gap_set``  the largest |synthetic - real NES| and its set's index (NaN and -1 without such a set)

    A share over an empty set and a correlation of a constant vector or of fewer than two sets are NaN."""
    nr, ns = np.asarray(real["nes"], dtype=np.float64), np.asarray(synth["nes"], dtype=np.float64)
    er, es = np.asarray(real["es"], dtype=np.float64), np.asarray(synth["es"], dtype=np.float64)
    qr, qs = np.asarray(real["q"], dtype=np.float64), np.asarray(synth["q"], dtype=np.float64)
    S = nr.shape[0]
    if S < 1 or any(a.shape != (S,) for a in (ns, er, es, qr, qs)):
        raise ValueError("one entry per set in every array")
    from scipy.stats import rankdata
    ok = np.isfinite(nr) & np.isfinite(ns)
    a, b = nr[ok], ns[ok]
    many = a.size >= 2
    ca = a - a.mean() if many else a
    var = float((ca * ca).sum()) if many else 0.0
    gap = np.where(ok, np.abs(ns - nr), -1.0)
    hr, hs = qr < alpha, qs < alpha
    return {
        "nes_pearson": DE._pearson(a, b) if many else float("nan"),
        "nes_spearman": DE._pearson(rankdata(a), rankdata(b)) if many else float("nan"),
        "nes_slope": float((ca * (b - b.mean())).sum() / var) if var > 0 else float("nan"),
        "sign_agreement": DE._share(np.sign(es[hr]) == np.sign(er[hr])),
        "real_hits": int(hr.sum()),
        "synth_hits": int(hs.sum()),
        "precision": DE._share(hr[hs]),
        "recall": DE._share(hs[hr]),
        "false_signal_share": DE._share(hs[qr > 0.5]),
        "max_abs_nes_gap": float(gap.max()) if ok.any() else float("nan"),
        "max_gap_set": int(np.argmax(gap)) if ok.any() else -1,
    }


def cohort_enrichment(k, x: torch.Tensor, labels: np.ndarray, sets: Sequence[np.ndarray], weight: float = 1.0, permutations: int = 1000,
                      seed: int = 0) -> Dict[str, np.ndarray]:
    """``enrichment_statistics`` of one cohort and contrast: the z of ``diffexp.cohort_statistics`` ranks the genes, one ``k.gsea``
    call scores the sets; ``stat``, ``pos``, ``size`` and the null's ``es_pos`` / ``es_neg`` ride along."""
    stat = DE.cohort_statistics(k, x, labels)["z"]
    pos = rank_positions(stat)
    res = k.gsea(position_weights(stat, pos, weight), [pos[np.asarray(m, dtype=np.int64)] for m in sets], int(permutations), int(seed))
    sizes = np.array([len(m) for m in sets], dtype=np.int64)
    out = enrichment_statistics(res["es_pos"], res["es_neg"], res["lead"], sizes)
    out.update(stat=stat, pos=pos, size=sizes, es_pos=res["es_pos"], es_neg=res["es_neg"])
    return out


def enrichment_metrics(k, x: torch.Tensor, real_cond: np.ndarray, y: torch.Tensor, synth_cond: np.ndarray, names: Sequence[str],
                       sets: Sequence[np.ndarray], weight: float = 1.0, permutations: int = 1000, alpha: float = 0.05, seed: int = 0,
                       sets_skipped: int = 0):
    """(summary, rows) over every column of the condition matrices [rows, K] (float64, host), the contrasts as in
    ``diffexp.differential_metrics``: per contrast with two non-empty groups in both cohorts the keys of ``enrichment_summary`` as
    ``gsea_<key>_<contrast>``, then ``gsea_<key>_mean`` over the contrasts for the keys of ``MEAN_KEYS`` (NaNs left out),
    ``gsea_contrasts``, ``gsea_skipped`` -- the contrasts with an empty group in either cohort, which add no other key --,
    ``gsea_sets`` and ``gsea_sets_skipped``.  ``sets``: per set its column indices.  ``rows[contrast]`` holds ``real`` and
    ``synthetic`` (``cohort_enrichment``) and ``threshold``."""
    summary: Dict[str, float] = {}
    rows: Dict[str, dict] = {}
    per_key = {key: [] for key in MEAN_KEYS}
    skipped = 0
    for j, name in enumerate(names):
        lr, ls, thr = DE.contrast_labels(real_cond[:, j], synth_cond[:, j])
        if min(int((lr == 1).sum()), int((lr == 0).sum()), int((ls == 1).sum()), int((ls == 0).sum())) < 1:
            skipped += 1
            continue
        real = cohort_enrichment(k, x, lr, sets, weight, permutations, seed)
        synth = cohort_enrichment(k, y, ls, sets, weight, permutations, seed)
        one = enrichment_summary(real, synth, alpha)
        summary.update({f"gsea_{key}_{name}": v for key, v in one.items()})
        for key in MEAN_KEYS:
            per_key[key].append(one[key])
        rows[name] = {"real": real, "synthetic": synth, "threshold": thr}
    for key, vals in per_key.items():
        live = [v for v in vals if not np.isnan(v)]
        if vals:
            summary[f"gsea_{key}_mean"] = float(np.mean(live)) if live else float("nan")
    summary["gsea_contrasts"] = len(names) - skipped
    summary["gsea_skipped"] = skipped
    summary["gsea_sets"] = len(sets)
    summary["gsea_sets_skipped"] = int(sets_skipped)
    return summary, rows
