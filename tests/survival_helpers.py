"""Float64 restatement of the survival kernels (csrc/cox.hip) and the planted cohorts the survival tests share.  Everything here
evaluates the SAME fp32 inputs the device sees -- features, centre, scale and weights are rounded to fp32 first -- in double, so a
difference to the device is the device's rounding alone."""
import functools

import numpy as np
import torch

from osteosarcoma_diffusionmodel_amd import survival as SV
from utility_helpers import NumpyKernels, _f32


def tie_groups(ts):
    """(gstart, gend) int arrays: the first and the last position of every position's run of equal values in the sorted ``ts``."""
    n = ts.size
    new = np.concatenate([[True], ts[1:] != ts[:-1]])
    gid = np.cumsum(new) - 1
    starts = np.nonzero(new)[0]
    ends = np.concatenate([starts[1:] - 1, [n - 1]])
    return starts[gid], ends[gid]


def cox_eval64(x, center, scale, w, time, event, round_w=True):
    """dict of float64 arrays for X [rows, D], the scan form of osd_val_cox_eval: ``loss`` (the negative Breslow partial
    log-likelihood, a sum), ``grad`` [D] and ``scores`` [rows]; the natural scale of each, what an error is measured against:
    ``loss_scale`` = sum_i delta_i |eta_i - m - log S_i|, ``grad_scale`` [D] = sum_j |r_j u_jc| and ``score_scale`` [rows] =
    sum_c |w_c u_ic|; and the pieces the rounding model needs: ``resid`` r [rows], ``u`` [rows, D], ``e`` [rows], ``risk`` S [rows]
    and ``c`` [rows].  A column with scale 0 is dropped: u = 0.  ``round_w=False`` takes w in double as it is."""
    x, c, s = _f32(x), _f32(center), _f32(scale)
    w = _f32(w) if round_w else np.asarray(w, dtype=np.float64)
    t, d = np.asarray(time, dtype=np.float64).ravel(), np.asarray(event, dtype=np.float64).ravel()
    rows = x.shape[0]
    u = (x - c) * s
    eta = u @ w
    m = eta.max()
    order = np.argsort(-t, kind="stable")                        # descending time, ties in row order
    gstart, gend = tie_groups(t[order])
    es, ds = np.exp(eta[order] - m), d[order]
    P = np.cumsum(es)
    S = P[gend]                                                  # the risk set, tied times included (Breslow)
    terms = ds * (eta[order] - m - np.log(S))
    q = ds / S
    Csuf = np.cumsum(q[::-1])[::-1]
    cs = Csuf[gstart]
    rs = -ds + es * cs
    back = np.empty(rows, dtype=np.int64)
    back[order] = np.arange(rows)
    r = rs[back]
    return {"loss": float(-terms.sum()), "grad": r @ u, "scores": eta, "loss_scale": float(np.abs(terms).sum()),
            "grad_scale": np.abs(r) @ np.abs(u), "score_scale": np.abs(u) @ np.abs(w), "resid": r, "u": u, "e": es[back],
            "risk": S[back], "c": cs[back]}


def cox_brute64(x, center, scale, w, time, event):
    """(loss, grad [D]) with the risk-set sums written directly, O(rows^2): for rows <= 300."""
    x, c, s, w = _f32(x), _f32(center), _f32(scale), _f32(w)
    t, d = np.asarray(time, dtype=np.float64).ravel(), np.asarray(event, dtype=np.float64).ravel()
    assert x.shape[0] <= 300
    u = (x - c) * s
    eta = u @ w
    m = eta.max()
    e = np.exp(eta - m)
    at_risk = t[None, :] >= t[:, None]                           # [i, k]: k is in i's risk set
    S = (at_risk * e[None, :]).sum(1)
    loss = -float((d * (eta - m - np.log(S))).sum())
    cj = ((t[:, None] <= t[None, :]) * (d / S)[:, None]).sum(0)  # [j]: sum over the events i with t_i <= t_j
    r = -d + e * cj
    return loss, r @ u


def concordance_loop(time, event, risk):
    """The four counts by the literal double loop."""
    t, d, r = (np.asarray(v, dtype=np.float64).ravel() for v in (time, event, risk))
    comp = conc = disc = tied = 0
    for i in range(t.size):
        if d[i] != 1.0:
            continue
        for j in range(t.size):
            if t[i] < t[j]:
                comp += 1
                conc += r[i] > r[j]
                disc += r[i] < r[j]
                tied += r[i] == r[j]
    return int(comp), int(conc), int(disc), int(tied)


class _Plan:
    def __init__(self, time, event):
        self.time, self.event = SV._survival_columns(time, event)      # the library's checks: finite times, flags 0 or 1
        self.rows, self.closed = self.time.size, False

    def close(self):
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SurvivalNumpyKernels(NumpyKernels):
    """``cox_plan``, ``cox_eval`` and ``concordance`` with the semantics of validation.DeviceKernels on CPU tensors, in double,
    beside the stand-ins of utility_helpers.NumpyKernels: the float64 pipeline is the validator's own host code over these."""

    @staticmethod
    def cox_plan(time, event):
        return _Plan(time, event)

    @staticmethod
    def cox_eval(x, center, scale, w, plan, grad=True, scores=False):
        assert not plan.closed and plan.rows == x.shape[0]
        r = cox_eval64(x, center, scale, w, plan.time, plan.event)
        return r["loss"], (r["grad"] if grad else None), (torch.from_numpy(r["scores"]) if scores else None)

    @staticmethod
    def concordance(time, event, risk):
        return SV.concordance_counts(_f32(time), _f32(event), _f32(risk))


def cox_eval_fn(x, center, scale, time, event, round_w=False):
    """The ``eval_fn`` of survival.fit_cox over one cohort, in double (w too, unless ``round_w``)."""
    def fn(w):
        r = cox_eval64(x, center, scale, w, time, event, round_w=round_w)
        return r["loss"], r["grad"]
    return fn


def penalised_cox_gradient64(x, center, scale, w, time, event, n, l2):
    """float64 gradient [D] of  loss / n + (l2 / 2) |w|^2  at w AS GIVEN (double, not rounded to fp32)."""
    w = np.asarray(w, dtype=np.float64)
    return cox_eval64(x, center, scale, w, time, event, round_w=False)["grad"] / n + l2 * w


def tie_grid(t, step=30.0):
    """Times rounded up to a multiple of ``step``: plentiful ties."""
    return np.ceil(np.asarray(t, dtype=np.float64) / step) * step


@functools.lru_cache(maxsize=None)
def cox_case(rows, D, ties="grid", seed=0):
    """Real-valued inputs of one kernel call: the features, centre and scale of utility_helpers.glm_case's recipe, weights of
    size 1 / sqrt(D), exponential times and about 35 % censoring.  ``ties``: "grid" (a 30-day grid), "distinct", "equal" (one
    time), "censored" (grid, no event), "events" (grid, no censoring), "fifty" (50 distinct times).  Returned arrays are shared
    between tests: copy before changing a value."""
    rs = np.random.default_rng(104729 * rows + 37 * D + 1000003 * seed)
    x = (rs.standard_normal((rows, D)) * (0.5 + rs.random(D)) + 3.0 * rs.standard_normal(D)).astype(np.float32)
    center = (x.astype(np.float64).mean(0) + 0.01 * rs.standard_normal(D)).astype(np.float32)
    scale = (1.0 / (0.5 + rs.random(D))).astype(np.float32)
    w = (rs.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    raw = rs.exponential(600.0, rows) + 1.0
    event = (rs.random(rows) < 0.65).astype(np.float64)
    if ties == "distinct":
        time = raw
        assert np.unique(time).size == rows
    elif ties == "equal":
        time = np.full(rows, 90.0)
    elif ties == "fifty":
        time = 30.0 * (1 + rs.integers(0, 50, rows)).astype(np.float64)
    else:
        time = tie_grid(raw)
    if ties == "censored":
        event = np.zeros(rows)
    elif ties == "events":
        event = np.ones(rows)
    return x, center, scale, w, time, event


@functools.lru_cache(maxsize=None)
def planted_survival(n=600, D=130, seed=3):
    """A cohort (features float32 [n, D], survival float64 [n, 2] = (time, event)) under proportional hazards: x ~ N(0, 1),
    eta = x0 - x1 + x2 / 2 - x3 / 2, event time ~ Exp(mean 800 exp(-eta)), censoring ~ Exp(mean 1600), the observed time rounded up
    to a multiple of 30 so that ties are plentiful."""
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n, D))
    eta = x[:, 0] - x[:, 1] + 0.5 * x[:, 2] - 0.5 * x[:, 3]
    t_event = rs.exponential(800.0 * np.exp(-eta))
    t_cens = rs.exponential(1600.0, n)
    event = (t_event <= t_cens).astype(np.float64)
    time = tie_grid(np.minimum(t_event, t_cens))
    return x.astype(np.float32), np.stack([time, event], axis=1)
