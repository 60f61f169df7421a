"""int64 / float64 NumPy restatement of ``osd_val_group_ranks`` (csrc/diffexp.hip) and a ``NumpyKernels`` stand-in with the semantics of
``validation.DeviceKernels.group_ranks``: the float64 pipeline is the package's own host code (``diffexp.differential_metrics``) over
these.

For one feature, a the case values sorted ascending (na of them), b the control values (nb of them), c the centre:
  u2      sum_i (#{b < a_i} + #{b <= a_i}), int64: twice the Mann-Whitney U of the cases over the controls, ties counted 1/2
  ties    sum of t^3 - t over the tie groups of the pooled column, int64, counted the kernel's way: a last-of-its-value element of a
          carries t = its run in a + (upper - lower bound in b), a last-of-its-value element of b whose value is not in a carries its
          run in b (the CPU tests hold this against the counts of np.unique)
  sum, sumsq   sum (x - c) and sum (x - c)^2 per group, float64
"""
import numpy as np
import torch

U52 = 2.0 ** -52


def _runs(v):
    """(index of the last element, length) of every run of equal values of the sorted vector v."""
    last = np.flatnonzero(np.append(v[1:] != v[:-1], True))
    return last, np.diff(np.append(-1, last))


def feature_ranks64(a, b):
    """(u2, ties) Python ints for two SORTED float64 columns."""
    lower, upper = np.searchsorted(b, a, side="left").astype(np.int64), np.searchsorted(b, a, side="right").astype(np.int64)
    u2 = int(lower.sum() + upper.sum())
    last_a, run_a = _runs(a)
    t = run_a.astype(np.int64) + (upper[last_a] - lower[last_a])
    ties = int((t ** 3 - t).sum())
    last_b, run_b = _runs(b)
    vb = b[last_b]
    pos = np.searchsorted(a, vb, side="left")
    absent = ~((pos < a.shape[0]) & (a[np.minimum(pos, a.shape[0] - 1)] == vb))
    t = run_b[absent].astype(np.int64)
    return u2, ties + int((t ** 3 - t).sum())


def group_ranks64(x, labels, center=None):
    """The restatement over all columns of x [rows, D] (fp32 values, evaluated in float64) with labels [rows] (1 a case, 0 a control,
    anything else ignored) and center [D] or None: the dictionary ``DeviceKernels.group_ranks`` returns."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    labels = np.asarray(labels)
    D = x.shape[1]
    c = np.zeros(D) if center is None else np.asarray(center, dtype=np.float32).astype(np.float64)
    a, b = np.sort(x[labels == 1], axis=0), np.sort(x[labels == 0], axis=0)
    if a.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError("a group is empty")
    ranks = [feature_ranks64(a[:, f], b[:, f]) for f in range(D)]
    da, db = a - c, b - c
    return {"u2": np.array([r[0] for r in ranks], dtype=np.int64), "ties": np.array([r[1] for r in ranks], dtype=np.int64),
            "sum": np.stack([da.sum(0), db.sum(0)]), "sumsq": np.stack([(da * da).sum(0), (db * db).sum(0)]),
            "sum_abs": np.stack([np.abs(da).sum(0), np.abs(db).sum(0)]), "na": int(a.shape[0]), "nb": int(b.shape[0])}


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


class NumpyKernels:
    """``group_ranks`` and ``col_centered_moments`` with the semantics of validation.DeviceKernels on CPU tensors, in double."""

    @staticmethod
    def group_ranks(t, labels, center=None, chunk_cols=0):
        r = group_ranks64(_np(t), _np(labels), None if center is None else _np(center))
        return {name: r[name] for name in ("u2", "ties", "sum", "sumsq", "na", "nb")}

    @staticmethod
    def col_centered_moments(t, center=None):
        d = _np(t).astype(np.float32).astype(np.float64) - (0.0 if center is None else _np(center).astype(np.float32).astype(np.float64))
        return d.sum(0), (d * d).sum(0)


# ---- planted cohorts: a known set of features differs between the groups ------------------------------------------------------------
def planted_effects(widths):
    """(E0, E1) float64 [D] for the blocks ``widths`` = (mutations, expression, pathways): the shift of every feature per unit of the
    binary condition (every fifth feature, +-0.8 in turn) and per unit of the continuous one (every seventh, +-0.8 in turn)."""
    D = int(sum(widths))
    e0, e1 = np.zeros(D), np.zeros(D)
    p0, p1 = np.arange(2, D, 5), np.arange(3, D, 7)
    e0[p0] = 0.8 * np.where(np.arange(p0.size) % 2 == 0, 1.0, -1.0)
    e1[p1] = 0.8 * np.where(np.arange(p1.size) % 2 == 0, 1.0, -1.0)
    return e0, e1


def planted_cohort(n, seed, widths, scale=1.0, flip=False, ignore=False):
    """(x fp32 [n, D], cond float64 [n, 2]): conditions (a binary one, 40 % cases, and a standard normal one) and features that
    follow them through the latent shift s = scale (E0 m + E1 z): binary mutations with rate 0.25 + 0.2 s, zero-inflated expression
    (30 % zeros, else a gamma value + s, floored at 0) and normal pathway scores + s.  ``flip``: the sign of E0 is reversed on every
    other planted feature; ``ignore``: the features follow conditions drawn afresh, not the ones returned."""
    n_mut, n_expr, n_pw = widths
    e0, e1 = planted_effects(widths)
    if flip:
        p0 = np.flatnonzero(e0)
        e0[p0[::2]] *= -1.0
    rs = np.random.default_rng(seed)
    cond = np.stack([(rs.random(n) < 0.4).astype(np.float64), rs.standard_normal(n)], axis=1)
    used = np.stack([(rs.random(n) < 0.4).astype(np.float64), rs.standard_normal(n)], axis=1) if ignore else cond
    s = scale * (used[:, :1] * e0 + used[:, 1:] * e1)
    mut = (rs.random((n, n_mut)) < np.clip(0.25 + 0.2 * s[:, :n_mut], 0.02, 0.98)).astype(np.float64)
    se = s[:, n_mut:n_mut + n_expr]
    expr = np.where(rs.random((n, n_expr)) < 0.3, 0.0, np.maximum(rs.gamma(2.0, 1.5, (n, n_expr)) + se, 0.0))
    pw = rs.standard_normal((n, n_pw)) + s[:, n_mut + n_expr:]
    return np.concatenate([mut, expr, pw], axis=1).astype(np.float32), cond


# ---- data kinds of the kernel tests -----------------------------------------------------------------------------------------------
KINDS = ["continuous", "binary", "zero_inflated", "eight_values", "all_equal", "disjoint", "signed_zeros"]
INTEGER_KINDS = ("binary", "eight_values", "all_equal")
ARRANGEMENTS = ["blocks", "alternating", "ignored"]


def make_groups(kind, na, nb, D, seed=0):
    """(cases fp32 [na, D], controls fp32 [nb, D]) of a data kind."""
    rs = np.random.default_rng(1000003 * seed + 7919 * na + 31 * nb + D + 13 * KINDS.index(kind))
    sa, sb = (na, D), (nb, D)
    if kind == "continuous":
        a = rs.standard_normal(sa) * (0.5 + rs.random(D)) + rs.standard_normal(D)
        b = rs.standard_normal(sb) * (0.5 + rs.random(D)) + rs.standard_normal(D)
    elif kind == "binary":
        a, b = rs.random(sa) < 0.3, rs.random(sb) < 0.45
    elif kind == "zero_inflated":                              # 30 % exact zeros and a gamma tail, as log2(counts + 1)
        a = np.where(rs.random(sa) < 0.3, 0.0, rs.gamma(2.0, 1.5, sa))
        b = np.where(rs.random(sb) < 0.3, 0.0, rs.gamma(2.2, 1.4, sb))
    elif kind == "eight_values":                               # eight integers: every value many times over
        a, b = rs.integers(-3, 5, sa), rs.integers(-3, 5, sb)
    elif kind == "all_equal":
        a, b = np.full(sa, 3.0), np.full(sb, 3.0)
    elif kind == "disjoint":                                   # even columns: every case above every control; odd columns: below
        a, b = rs.random(sa) + 2.0, rs.random(sb)
        a[:, 1::2] -= 4.0
    elif kind == "signed_zeros":                               # -0.0 and +0.0 compare equal and sort apart; a few other values around
        pick = lambda shape: rs.choice(np.array([-0.0, 0.0, -1.0, 1.0]), size=shape, p=[0.4, 0.4, 0.1, 0.1])
        a, b = pick(sa), pick(sb)
    else:
        raise ValueError(kind)
    return np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)


def arrange(a, b, how):
    """(x fp32 [rows, D], labels int32 [rows]) holding the cases a and the controls b: ``blocks`` all cases, then all controls;
    ``alternating`` case, control, case, ... until one group runs out; ``ignored`` the alternating order with a row of 1000s
    labelled -1 or 2 (in turn) after every third row."""
    na, nb = a.shape[0], b.shape[0]
    x = np.concatenate([a, b])
    labels = np.concatenate([np.ones(na, dtype=np.int32), np.zeros(nb, dtype=np.int32)])
    if how == "blocks":
        return x, labels
    order = np.argsort(np.concatenate([2 * np.arange(na), 2 * np.arange(nb) + 1]), kind="stable")
    x, labels = x[order], labels[order]
    if how == "alternating":
        return x, labels
    if how != "ignored":
        raise ValueError(how)
    n = na + nb
    rows = n + n // 3 + 1                                      # every fourth row and the last one are ignored: n rows are left
    ignored = (np.arange(rows) % 4 == 3) | (np.arange(rows) == rows - 1)
    xs = np.full((rows, x.shape[1]), 1000.0, dtype=np.float32)
    ls = np.where(np.cumsum(ignored) % 2 == 1, -1, 2).astype(np.int32)
    xs[~ignored], ls[~ignored] = x, labels
    return xs, ls
