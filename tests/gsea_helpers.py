"""float64 NumPy restatement of ``osd_val_gsea`` (csrc/gsea.hip) and a ``NumpyKernels`` stand-in that adds ``.gsea`` to the one of
tests/diffexp_helpers.py: the float64 pipeline is the package's own host code (``enrichment.enrichment_metrics``) over these.

For a set with the hit positions h_0 < ... < h_{k-1} in a list of D positions with the weights w:
  C_j = w[h_0] + ... + w[h_j] (np.cumsum: one after another), NR = C_{k-1}
  up_j = C_j / NR - (h_j - j) / (D - k),  dn_j = C_{j-1} / NR - (h_j - j) / (D - k)   ((j + 1) / k and j / k for the ratios when NR == 0)
  ES+ = max up_j, ES- = min dn_j, lead = (argmax, argmin): the first hit numbers that attain them
Permutation p >= 1 moves position i to the rank of (key_p(i), i), key_p(i) word 0 of the Philox block at (seed; i, p, 0, TAG_GSEA)."""
import numpy as np

from diffexp_helpers import NumpyKernels as _DiffexpKernels
from diffexp_helpers import planted_effects
from helpers import philox4x32_10

TAG_GSEA = 0x47534500


def perm_keys(seed, p, D):
    """uint32 [D]: the sort keys of permutation p."""
    return philox4x32_10(np.arange(D, dtype=np.uint32), np.uint32(p), np.uint32(0), np.uint32(TAG_GSEA), seed & 0xFFFFFFFF,
                         (seed >> 32) & 0xFFFFFFFF)[0]


def perm_ranks(seed, p, D):
    """int64 [D]: rho_p(i), the rank of (key_p(i), i) -- a stable argsort of the keys breaks ties by the smaller index; p = 0 is the
    identity."""
    if p == 0:
        return np.arange(D, dtype=np.int64)
    order = np.argsort(perm_keys(seed, p, D), kind="stable")
    rho = np.empty(D, dtype=np.int64)
    rho[order] = np.arange(D, dtype=np.int64)
    return rho


def es_pair(w, hits, D):
    """(ES+, ES-, first hit number of the maximum, of the minimum) for the hit positions ``hits`` (any order, distinct)."""
    h = np.sort(np.asarray(hits, dtype=np.int64))
    k = h.shape[0]
    j = np.arange(k, dtype=np.int64)
    c = np.cumsum(np.asarray(w, dtype=np.float64)[h])
    nr = c[-1]
    if nr == 0.0:
        hit, prev = (j + 1).astype(np.float64) / np.float64(k), j.astype(np.float64) / np.float64(k)
    else:
        hit, prev = c / nr, np.concatenate([[0.0], c[:-1]]) / nr
    miss = (h - j).astype(np.float64) / np.float64(D - k)
    up, dn = hit - miss, prev - miss
    ju, jd = int(np.argmax(up)), int(np.argmin(dn))
    return up[ju], dn[jd], ju, jd


def gsea64(weights, set_positions, permutations, seed):
    """The restatement: the dictionary ``DeviceKernels.gsea`` returns."""
    w = np.asarray(weights, dtype=np.float64)
    D, S = w.shape[0], len(set_positions)
    es_pos, es_neg = np.zeros((permutations + 1, S)), np.zeros((permutations + 1, S))
    lead = np.zeros((S, 2), dtype=np.int32)
    sets = [np.asarray(m, dtype=np.int64) for m in set_positions]
    for p in range(permutations + 1):
        rho = perm_ranks(seed, p, D)
        for s, m in enumerate(sets):
            es_pos[p, s], es_neg[p, s], ju, jd = es_pair(w, rho[m], D)
            if p == 0:
                lead[s] = (ju, jd)
    return {"es_pos": es_pos, "es_neg": es_neg, "lead": lead}


class NumpyKernels(_DiffexpKernels):
    """``group_ranks``, ``col_centered_moments`` and ``gsea`` with the semantics of validation.DeviceKernels, in double."""

    @staticmethod
    def gsea(weights, set_positions, permutations, seed=0, perm_chunk=0):
        return gsea64(weights, set_positions, permutations, seed)


# ---- the planted gene sets of the end-to-end tests: the expression slice 20:110 of planted_cohort's widths (20, 90, 20) ------------
WIDTHS = (20, 90, 20)
EXPR = slice(20, 110)


def planted_sets():
    """An ordered {name: column indices of the expression slice}: UP the 9 genes the binary condition raises + 3 null genes, DOWN the
    9 it lowers + 3 null, MIXED 4 + 4 + 4 null, NULL_A and NULL_B 12 null genes each, BIG 40 of the 90 genes, SMALL 5 null genes."""
    e0 = planted_effects(WIDTHS)[0][EXPR]
    up, down, null = np.flatnonzero(e0 > 0), np.flatnonzero(e0 < 0), np.flatnonzero(e0 == 0)
    rs = np.random.default_rng(3)
    sets = {"UP": np.concatenate([up, null[:3]]), "DOWN": np.concatenate([down, null[3:6]]),
            "MIXED": np.concatenate([up[:4], down[:4], null[6:10]])}
    sets["NULL_A"] = rs.choice(null, 12, replace=False)
    sets["NULL_B"] = rs.choice(null, 12, replace=False)
    sets["BIG"] = rs.choice(90, 40, replace=False)
    sets["SMALL"] = null[10:15]
    return sets
