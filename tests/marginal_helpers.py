"""float64 / int64 NumPy restatement of ``osd_val_marginals`` (csrc/marginal.hip) and a ``NumpyKernels`` stand-in with the semantics of
``validation.DeviceKernels``: the float64 pipeline is the validator's own host code (``sharded_marginals``, ``real_sample_sd``,
``marginal_summary``) over these.

For one feature, a the real column sorted ascending (n1 values), b the synthetic one (n2 values):
  KS extremes   max / min over the pooled sample points v of #{a <= v} n2 - #{b <= v} n1, int64
  W1            (1 / (n1 n2)) sum |a_i - b_j| w_ij over the quantile coupling: the n1 n2 unit cells of [0, n1 n2) are cut at the
                multiples of n2 (the real quantile steps) and of n1 (the synthetic ones); a piece that starts at cut p has length
                w = next cut - p, belongs to real value i = p // n2 and synthetic value j = p // n1 -- the same (i, j, w_ij) as
                i = 0 .. n1 - 1, j = floor(i n2 / n1) .. floor(((i + 1) n2 - 1) / n1), w_ij = min((i + 1) n2, (j + 1) n1) - max(i n2, j n1)
  below, above  #{b < a_0}, #{b > a_(n1 - 1)}
"""
import numpy as np
import torch

U52 = 2.0 ** -52


def coupling(n1, n2):
    """(i, j, w) int64 arrays: the pairs of the quantile coupling with their integer weights, in order; w sums to n1 n2."""
    cuts = np.union1d(np.arange(n1, dtype=np.int64) * n2, np.arange(n2, dtype=np.int64) * n1)
    w = np.diff(np.append(cuts, np.int64(n1) * np.int64(n2)))
    return cuts // n2, cuts // n1, w


def ks_extremes64(a, b):
    """(dmax, dmin) Python ints for two sorted float64 columns."""
    n1, n2 = a.shape[0], b.shape[0]
    pooled = np.concatenate([a, b])
    d = np.searchsorted(a, pooled, side="right").astype(np.int64) * n2 - np.searchsorted(b, pooled, side="right").astype(np.int64) * n1
    return int(d.max()), int(d.min())


def marginals64(real, synth, integer=False):
    """The restatement over all columns of two [n, D] arrays (fp32 values, evaluated in float64): a dict of ``ks_dmax``, ``ks_dmin``,
    ``below``, ``above`` (int64 [D]) and ``w1`` (float64 [D]); with ``integer=True`` (integer-valued data) also ``w1_int``, the exact
    int64 sums  sum |a_i - b_j| w_ij."""
    a = np.sort(np.asarray(real, dtype=np.float64), axis=0)
    b = np.sort(np.asarray(synth, dtype=np.float64), axis=0)
    (n1, D), n2 = a.shape, b.shape[0]
    ext = [ks_extremes64(a[:, f], b[:, f]) for f in range(D)]
    i, j, w = coupling(n1, n2)
    diff = np.ascontiguousarray(np.abs(a[i] - b[j]).T)                      # [D, pairs]: numpy adds the contiguous axis pairwise
    out = {"ks_dmax": np.array([e[0] for e in ext], dtype=np.int64), "ks_dmin": np.array([e[1] for e in ext], dtype=np.int64),
           "w1": (diff * w.astype(np.float64)).sum(1) / (float(n1) * float(n2)),
           "below": (b < a[0]).sum(0).astype(np.int64), "above": (b > a[-1]).sum(0).astype(np.int64)}
    if integer:
        out["w1_int"] = (np.rint(diff).astype(np.int64) * w).sum(1)
    return out


def _f32(v):
    return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32).astype(np.float64)


class NumpyKernels:
    """``marginals`` and ``col_centered_moments`` with the semantics of validation.DeviceKernels on CPU tensors, in double."""

    @staticmethod
    def marginals(real, synth, chunk_cols=0):
        r = marginals64(_f32(real), _f32(synth))
        return {name: r[name] for name in ("ks_dmax", "ks_dmin", "w1", "below", "above")}

    @staticmethod
    def col_centered_moments(t, center=None):
        d = _f32(t) - (0.0 if center is None else _f32(center))
        return d.sum(0), (d * d).sum(0)


# ---- data kinds of the kernel tests -----------------------------------------------------------------------------------------------
KINDS = ["normal", "ties", "zero_inflated", "binary", "signed_zeros", "constant_column", "identical", "disjoint"]
INTEGER_KINDS = ("ties", "binary")


def make_case(kind, n1, n2, D, seed=0):
    """(real fp32 [n1, D], synth fp32 [n2, D]) of a data kind; ``identical`` needs nothing of n2 (the caller passes n2 = n1)."""
    rs = np.random.default_rng(1000003 * seed + 7919 * n1 + 31 * n2 + D + 13 * KINDS.index(kind))
    shape_a, shape_b = (n1, D), (n2, D)
    if kind == "normal":
        a = rs.standard_normal(shape_a) * (0.5 + rs.random(D)) + rs.standard_normal(D)
        b = rs.standard_normal(shape_b) * (0.5 + rs.random(D)) + rs.standard_normal(D)
    elif kind == "ties":                                       # small integers: every value many times over
        a, b = rs.integers(-3, 4, shape_a), rs.integers(-2, 6, shape_b)
    elif kind == "zero_inflated":                              # 30 % exact zeros and a gamma tail
        a = np.where(rs.random(shape_a) < 0.3, 0.0, rs.gamma(2.0, 1.5, shape_a))
        b = np.where(rs.random(shape_b) < 0.3, 0.0, rs.gamma(2.2, 1.4, shape_b))
    elif kind == "binary":
        a, b = rs.random(shape_a) < 0.3, rs.random(shape_b) < 0.45
    elif kind == "signed_zeros":                               # -0.0 and +0.0 compare equal and sort apart; a few other values around
        pick = lambda shape: rs.choice(np.array([-0.0, 0.0, -1.0, 1.0]), size=shape, p=[0.4, 0.4, 0.1, 0.1])
        a, b = pick(shape_a), pick(shape_b)
    elif kind == "constant_column":                            # the middle column constant in the real cohort, and column 0 in both
        a, b = rs.standard_normal(shape_a), rs.standard_normal(shape_b)
        a[:, D // 2] = 2.5
        a[:, 0], b[:, 0] = -1.25, -1.25
    elif kind == "identical":
        a = rs.standard_normal(shape_a)
        a[:, D // 2] = np.round(a[:, D // 2])
        b = a[rs.permutation(n1)]                              # the same values in another row order
    elif kind == "disjoint":                                   # even columns: synthetic above the real range; odd columns: below
        a, b = rs.random(shape_a), rs.random(shape_b) + 2.0
        b[:, 1::2] -= 4.0
    else:
        raise ValueError(kind)
    return np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
