"""Float64 restatement of the univariate Cox screen kernel (csrc/cox_score.hip) and the stand-in kernels the prognostic tests share.
As in survival_helpers.py everything evaluates the SAME fp32 inputs the device sees -- features, centre and scale are rounded to fp32
first; beta and the bound are doubles on the device too -- in double, so a difference to the device is the device's rounding alone."""
import numpy as np

from survival_helpers import SurvivalNumpyKernels, tie_groups
from utility_helpers import _f32


def _inputs(x, center, scale, time, event, beta, bound):
    x, c, s = _f32(x), _f32(center), _f32(scale)
    t, d = np.asarray(time, dtype=np.float64).ravel(), np.asarray(event, dtype=np.float64).ravel()
    D = x.shape[1]
    u = (x - c) * s
    b = np.zeros(D) if beta is None else np.asarray(beta, dtype=np.float64).reshape(D)
    R = np.zeros(D) if bound is None else np.asarray(bound, dtype=np.float64).reshape(D)
    arg = b * u - np.abs(b) * R                                  # the device's order: the product, then the shift
    e = np.ones_like(u) if beta is None else np.exp(arg)
    return u, arg, e, t, d, s == 0


def cox_score64(x, center, scale, time, event, beta=None, bound=None):
    """dict of float64 [D] arrays for X [rows, D], the scan form of osd_val_cox_score: ``loglik``, ``score``, ``info``, ``absmax``;
    what an error of each is measured against, the sum of the absolute values of the terms it adds and subtracts -- ``loglik_scale`` =
    sum_p delta_p (|beta u - k| + |log A0|), ``score_scale`` = sum_p delta_p (|u| + |A1 / A0|), ``info_scale`` = sum_p delta_p
    (A2 / A0 + (A1 / A0)^2); and what the rounding model needs: ``events`` (a number), ``max_arg`` = max |beta u - k| and
    ``spread1`` = sum_p delta_p B1 / A0, ``spread2`` = sum_p delta_p |A1 / A0| B1 / A0 with B1 the risk-set sum of e |u| (what an error
    of the running sums is relative to).  A column with scale 0 is dropped: zeros everywhere."""
    u, arg, e, t, d, dropped = _inputs(x, center, scale, time, event, beta, bound)
    order = np.argsort(-t, kind="stable")                        # descending time, ties in row order
    _, gend = tie_groups(t[order])
    uo, eo, ao, dd = u[order], e[order], arg[order], d[order][:, None]
    A0, A1, A2 = np.cumsum(eo, 0)[gend], np.cumsum(eo * uo, 0)[gend], np.cumsum(eo * uo * uo, 0)[gend]
    B1 = np.cumsum(eo * np.abs(uo), 0)[gend]
    m1, m2, logA0 = A1 / A0, A2 / A0, np.log(A0)
    out = {"loglik": (dd * (ao - logA0)).sum(0), "score": (dd * (uo - m1)).sum(0), "info": (dd * (m2 - m1 * m1)).sum(0),
           "absmax": np.abs(u).max(0),
           "loglik_scale": (dd * (np.abs(ao) + np.abs(logA0))).sum(0), "score_scale": (dd * (np.abs(uo) + np.abs(m1))).sum(0),
           "info_scale": (dd * (m2 + m1 * m1)).sum(0), "spread1": (dd * B1 / A0).sum(0), "spread2": (dd * np.abs(m1) * B1 / A0).sum(0)}
    for v in out.values():
        v[dropped] = 0.0
    out["events"], out["max_arg"] = float(d.sum()), float(np.abs(arg).max())
    return out


def cox_score_brute64(x, center, scale, time, event, beta=None, bound=None):
    """(loglik, score, info) [D] with the risk-set sums written directly, O(rows^2 D): for rows <= 300."""
    u, arg, e, t, d, dropped = _inputs(x, center, scale, time, event, beta, bound)
    assert u.shape[0] <= 300
    at_risk = (t[None, :] >= t[:, None]).astype(np.float64)      # [i, k]: k is in i's risk set
    A0, A1, A2 = at_risk @ e, at_risk @ (e * u), at_risk @ (e * u * u)
    dd = d[:, None]
    out = [(dd * (arg - np.log(A0))).sum(0), (dd * (u - A1 / A0)).sum(0), (dd * (A2 / A0 - (A1 / A0) ** 2)).sum(0)]
    for v in out:
        v[dropped] = 0.0
    return tuple(out)


def logrank_chi2(group, time, event):
    """The textbook log-rank chi-square of a 0/1 covariate: (O1 - E1)^2 / V with, over the distinct event times, d events among n at
    risk, n1 of them in group 1: E1 = sum d n1 / n, V = sum d (n1 / n) (1 - n1 / n) (n - d) / (n - 1) -- observed minus expected over
    the hypergeometric variances."""
    g, t, d = (np.asarray(v, dtype=np.float64).ravel() for v in (group, time, event))
    o1 = e1 = var = 0.0
    for s in np.unique(t[d == 1.0]):
        at = t >= s
        n, n1 = float(at.sum()), float((at & (g == 1.0)).sum())
        here = (t == s) & (d == 1.0)
        dj = float(here.sum())
        o1 += float((here & (g == 1.0)).sum())
        e1 += dj * n1 / n
        if n > 1:
            var += dj * (n1 / n) * (1.0 - n1 / n) * (n - dj) / (n - 1.0)
    return (o1 - e1) ** 2 / var


class PrognosticNumpyKernels(SurvivalNumpyKernels):
    """``cox_score`` with the semantics of validation.DeviceKernels on CPU tensors, in double, beside the stand-ins it inherits."""

    @staticmethod
    def cox_score(x, center, scale, plan, beta=None, bound=None, absmax=False):
        assert not plan.closed and plan.rows == x.shape[0]
        r = cox_score64(x, center, scale, plan.time, plan.event, beta, bound)
        return r["loglik"], r["score"], r["info"], (r["absmax"] if absmax else None)


def score_eval_fn(x, center, scale, time, event, bound):
    """The ``eval_fn`` of survival.univariate_cox over one cohort, in double."""
    def fn(beta):
        r = cox_score64(x, center, scale, time, event, beta, bound)
        return r["loglik"], r["score"], r["info"]
    return fn
