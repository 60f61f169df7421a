"""float64 NumPy restatement of ``osd_val_pathway_scores`` and ``osd_val_pathway_agreement`` (csrc/pathway.hip) and a ``NumpyKernels``
stand-in that adds ``.pathway_scores`` and ``.pathway_agreement`` to the one of tests/gsea_helpers.py: the float64 pipeline is the
package's own host code (``pathways.PathwayScorer``, ``pathways.pathway_consistency``) over these.

For one row x (fp32 values, evaluated in float64) and a set of m distinct columns:
  mean     (sum_j (x_j - c_j) s_j) / m,   zscore   (sum_j (x_j - c_j) s_j) / sqrt(m)      -- np.cumsum: one after another
  ssgsea   r = scipy's rankdata(method="average") of the row (1 ... D; -0.0 == +0.0; +-inf as values), T[k] = (k / 2) ** alpha made on
           the host,  ES = sum_j r_j T[2 r_j] / sum_j T[2 r_j] - (D (D + 1) / 2 - sum_j r_j) / (D - m);  a row with a NaN: all NaN
``literal_walk`` is the definition the closed form integrates: the weighted running sum over the descending order, summed over its
positions."""
import numpy as np
import torch
from scipy.stats import rankdata

from gsea_helpers import NumpyKernels as _GseaKernels

U53 = 2.0 ** -53
METHODS = ("mean", "zscore", "ssgsea")


def rank_table(D, alpha=0.25):
    """float64 [2 D + 1]: T[k] = (k / 2) ** alpha."""
    return np.power(np.arange(2 * int(D) + 1, dtype=np.float64) / 2.0, float(alpha))


def _seq_sum(a):
    """The sum along the last axis, one term after another."""
    return np.cumsum(a, axis=-1)[..., -1]


def linear64(x, sets, method, center=None, scale=None):
    """(scores float64 [rows, S], abs float64 [rows, S]: norm * sum_j |(x_j - c_j) s_j|, what the tolerance scales with)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    D = x.shape[1]
    c = np.zeros(D) if center is None else np.asarray(center, dtype=np.float32).astype(np.float64)
    s = np.ones(D) if scale is None else np.asarray(scale, dtype=np.float32).astype(np.float64)
    out, mag = np.zeros((x.shape[0], len(sets))), np.zeros((x.shape[0], len(sets)))
    with np.errstate(invalid="ignore", over="ignore"):
        for q, m in enumerate(sets):
            m = np.asarray(m, dtype=np.int64)
            term = (x[:, m] - c[m]) * s[m]
            norm = float(m.size) if method == "mean" else np.sqrt(np.float64(m.size))
            out[:, q], mag[:, q] = _seq_sum(term) / norm, _seq_sum(np.abs(term)) / norm
    return out, mag


def midranks(x):
    """float64 [rows, D]: every row's ascending mid-ranks; a row with a NaN is all NaN."""
    x = np.asarray(x, dtype=np.float32)
    bad = np.isnan(x).any(axis=1)
    r = rankdata(np.where(bad[:, None], np.float32(0), x), method="average", axis=1).astype(np.float64)
    r[bad] = np.nan
    return r


def ssgsea64(x, sets, table):
    """scores float64 [rows, S] by the closed form over scipy's mid-ranks."""
    r = midranks(x)
    rows, D = r.shape
    bad = np.isnan(r[:, 0])
    r2 = np.where(bad[:, None], 2, np.rint(2.0 * r)).astype(np.int64)
    out = np.zeros((rows, len(sets)))
    for q, m in enumerate(sets):
        m = np.asarray(m, dtype=np.int64)
        rm, t = 0.5 * r2[:, m], table[r2[:, m]]
        out[:, q] = _seq_sum(rm * t) / _seq_sum(t) - (D * (D + 1) / 2.0 - _seq_sum(rm)) / float(D - m.size)
    out[bad] = np.nan
    return out


def literal_walk(x, members, alpha):
    """The enrichment score of one untied row by its definition: genes in descending order, P_hit(i) the weighted share of the
    set's genes among the first i (weight: ascending rank ** alpha), P_miss(i) the share of the other genes; the sum over i of
    P_hit(i) - P_miss(i)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    D = x.shape[0]
    order = np.argsort(-x, kind="stable")
    rank = np.empty(D)
    rank[order] = np.arange(D, 0, -1, dtype=np.float64)            # ascending rank: the largest value has D
    inset = np.zeros(D, dtype=bool)
    inset[np.asarray(members, dtype=np.int64)] = True
    w = np.where(inset[order], rank[order] ** float(alpha), 0.0)
    p_hit = np.cumsum(w) / w.sum()
    p_miss = np.cumsum(~inset[order]) / float(D - inset.sum())
    return float(np.sum(p_hit - p_miss))


def scores64(x, sets, method, center=None, scale=None, table=None):
    if method == "ssgsea":
        return ssgsea64(x, sets, table)
    return linear64(x, sets, method, center, scale)[0]


def agreement64(scores, block, mu, isd):
    """(sums float64 [S, 6], used int64 [S], abs float64 [S, 6]: the sums of the terms' magnitudes)."""
    p = np.asarray(scores, dtype=np.float64)
    S = p.shape[1]
    g = np.asarray(block, dtype=np.float32).astype(np.float64)[:, :S]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (p - np.asarray(mu, dtype=np.float64)) * np.asarray(isd, dtype=np.float64)
        ok = np.isfinite(z) & np.isfinite(g)
        z, g = np.where(ok, z, 0.0), np.where(ok, g, 0.0)
        terms = np.stack([z, g, z * z, g * g, z * g, (g - z) * (g - z)], axis=2)
    return terms.sum(axis=0), ok.sum(axis=0).astype(np.int64), np.abs(terms).sum(axis=0)


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


class NumpyKernels(_GseaKernels):
    """``pathway_scores`` and ``pathway_agreement`` with the semantics of validation.DeviceKernels on CPU tensors, in double, beside
    the stand-ins of the other helpers (``col_centered_moments`` among them).  ``device``: where a scorer puts its tensors."""
    device = torch.device("cpu")

    @staticmethod
    def pathway_scores(t, sets, method="mean", center=None, scale=None, rank_table=None, row_chunk=0, phases=False):
        if method not in METHODS:
            raise ValueError(method)
        if method == "ssgsea" and rank_table is None:
            raise ValueError("ssgsea needs rank_table")
        out = scores64(_np(t), sets, method, None if center is None else _np(center), None if scale is None else _np(scale), rank_table)
        return torch.from_numpy(out)

    @staticmethod
    def pathway_agreement(scores, block, mu, isd):
        sums, used, _ = agreement64(_np(scores), _np(block), mu, isd)
        return {"sums": sums, "used": used}


# ---- data kinds of the kernel tests -----------------------------------------------------------------------------------------------
KINDS = ["continuous", "zero_inflated", "all_equal", "integers", "infinities", "nan_row"]


def make_rows(kind, rows, D, seed=0):
    """x fp32 [rows, D] of a data kind."""
    rs = np.random.default_rng(7919 * seed + 131 * rows + D + 17 * KINDS.index(kind))
    if kind in ("continuous", "infinities"):
        x = rs.standard_normal((rows, D)) * 2.0 + 1.0
        if kind == "infinities":                               # one +inf and one -inf in every row
            cols = np.stack([rs.permutation(D)[:2] for _ in range(rows)])
            x[np.arange(rows), cols[:, 0]], x[np.arange(rows), cols[:, 1]] = np.inf, -np.inf
    elif kind in ("zero_inflated", "nan_row"):                 # 30 % exact zeros, a -0.0 among them, and a gamma tail
        x = np.where(rs.random((rows, D)) < 0.3, 0.0, rs.gamma(2.0, 1.5, (rows, D)))
        x[np.arange(rows), rs.integers(0, D, rows)] = -0.0
        if kind == "nan_row":
            x[rows // 2, int(rs.integers(0, D))] = np.nan
    elif kind == "all_equal":
        x = np.full((rows, D), 3.0)
    elif kind == "integers":
        x = rs.integers(0, 4, (rows, D)).astype(np.float64)
    else:
        raise ValueError(kind)
    return np.asarray(x, dtype=np.float32)


def make_sets(D, sizes, seed=0):
    """One set of distinct columns per size, drawn independently (so they overlap)."""
    rs = np.random.default_rng(104729 * seed + D)
    return [rs.permutation(D)[:m].astype(np.int64) for m in sizes]


def covering_sets(D, m):
    """Sets of m columns that together use every column (U = D), in a shuffled order."""
    perm = np.random.default_rng(D).permutation(D)
    sets = [perm[i:i + m] for i in range(0, D - m + 1, m)]
    if D % m:
        sets.append(perm[D - m:])
    return [s.astype(np.int64) for s in sets]


# ---- the planted cohorts of the consistency tests ------------------------------------------------------------------------------------
N_REAL, N_SYNTH, N_GENES, SEED = 600, 900, 90, 7
SET_SIZES = (5, 9, 17, 30, 45, 60, 89)


def planted_sets():
    """An ordered {name: column indices}: seven sets of 5 - 89 of the 90 genes."""
    rs = np.random.default_rng(SEED)
    return {f"SET_{m}": np.sort(rs.permutation(N_GENES)[:m]).astype(np.int64) for m in SET_SIZES}


def planted_expression(n, seed):
    """fp32 [n, 90]: zero-inflated expression (30 % zeros, a gamma tail) with a per-patient activity that moves the genes together."""
    rs = np.random.default_rng(seed)
    activity = rs.standard_normal((n, 1))
    load = np.random.default_rng(SEED + 1).random(N_GENES)        # the same genes respond in every cohort
    x = np.maximum(rs.gamma(2.0, 1.5, (n, N_GENES)) + activity * load, 0.0)
    return np.where(rs.random((n, N_GENES)) < 0.3, 0.0, x).astype(np.float32)


def planted_cohorts(method, alpha=0.25):
    """The design of the consistency tests for one method: ``real`` and ``synth`` expression, ``sets``, ``real_block`` (the real
    cohort's standardised scores, fp32), ``z`` (the synthetic cohort's standardised scores by the float64 stand-in), ``faithful`` =
    z + 0.1 N(0, 1) (fp32) and ``decoupled``, the same block with its rows permuted."""
    from osteosarcoma_diffusionmodel_amd.pathways import PathwayScorer
    real, synth = planted_expression(N_REAL, SEED), planted_expression(N_SYNTH, SEED + 100)
    sets = planted_sets()
    scorer = PathwayScorer(sets, list(range(N_GENES)), method=method, alpha=alpha, kernels=NumpyKernels()).fit(real)
    z = scorer.score(synth, standardize=True).numpy()
    rs = np.random.default_rng(SEED + 2)
    faithful = (z + 0.1 * rs.standard_normal(z.shape)).astype(np.float32)
    return {"real": real, "synth": synth, "sets": sets, "names": list(sets), "z": z, "faithful": faithful,
            "decoupled": faithful[rs.permutation(N_SYNTH)], "real_block": scorer.score(real, standardize=True).numpy().astype(np.float32)}
