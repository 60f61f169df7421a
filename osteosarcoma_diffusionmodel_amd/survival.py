"""Survival utility, host side: the driver that fits an L2-regularised Cox proportional-hazards model
through an ``eval_fn`` -- the device kernels behind ``DeviceKernels.cox_eval`` or a float64 restatement, the driver cannot tell --,
Harrell's concordance as exact pair counts, and the summary that turns two fits and their counts into the ``survival_*`` result keys
of ``BiologicalValidator.survival_utility``.  numpy float64 throughout; no device code: this module imports on a machine without a
GPU."""
from __future__ import annotations

from typing import Callable, Dict, Mapping, Sequence, Tuple

import numpy as np

from .utility import _lbfgs


def fit_cox(eval_fn: Callable[[np.ndarray], Tuple[float, np.ndarray]], D: int, n: float, l2: float, max_iter: int = 200,
            tol: float = 1e-5, history: int = 10) -> Dict[str, object]:
    """Minimise  F(w) = loss(w) / n + (l2 / 2) |w|^2  over w [D] by the L-BFGS of ``utility.fit_glm`` (the same loop), from w = 0.
    ``eval_fn(w) -> (loss, grad [D])`` returns the negative Breslow partial log-likelihood and its gradient as SUMS over the rows, as
    ``osd_val_cox_eval`` does, and is all the driver knows about the data; ``n`` is the row count.  There is no intercept: the partial
    likelihood does not see one.  A non-finite loss (a step whose scores underflow a whole risk set) is a rejected line-search step.

    Returns ``{"w", "iterations", "converged", "grad_inf_norm"}``: converged means the gradient's infinity norm fell to ``tol``; a
    line search that finds no Armijo step ends the fit with ``converged=False``, nothing is raised."""
    D = int(D)
    if D < 1:
        raise ValueError("fit_cox needs D >= 1 features")
    if not (n > 0 and l2 >= 0 and max_iter >= 0 and history >= 1):
        raise ValueError("fit_cox needs n > 0, l2 >= 0, max_iter >= 0 and history >= 1")
    n, l2 = float(n), float(l2)

    def objective(w):
        loss, grad = eval_fn(w)
        grad = np.asarray(grad, dtype=np.float64).reshape(D)
        return float(loss) / n + 0.5 * l2 * float(w @ w), grad / n + l2 * w

    w, it, converged, gnorm = _lbfgs(objective, np.zeros(D, dtype=np.float64), max_iter, tol, history)
    return {"w": w.copy(), "iterations": it, "converged": converged, "grad_inf_norm": gnorm}


def _survival_columns(time, event, risk=None):
    t, d = np.asarray(time, dtype=np.float64).ravel(), np.asarray(event, dtype=np.float64).ravel()
    if t.size == 0 or d.shape != t.shape:
        raise ValueError("one event flag per time, and at least one row")
    if not np.isfinite(t).all() or not np.isin(d, (0.0, 1.0)).all():
        raise ValueError("times must be finite and event flags 0 or 1")
    if risk is None:
        return t, d
    r = np.asarray(risk, dtype=np.float64).ravel()
    if r.shape != t.shape or not np.isfinite(r).all():
        raise ValueError("one finite risk per row")
    return t, d, r


def concordance_counts(time, event, risk, chunk: int = 1024) -> Tuple[int, int, int, int]:
    """Exact pair counts of Harrell's concordance, as ``osd_val_concordance`` returns them: over the ordered pairs (i, j) with
    event_i = 1 and time_i < time_j (strict: equal times are not comparable) ``(comparable, concordant, discordant, tied_risk)`` --
    risk_i > risk_j, risk_i < risk_j, risk_i == risk_j.  Rows are sorted by time, so the partners of i are a suffix; ``chunk`` events
    are compared against their suffixes at a time (O(n^2) comparisons, O(chunk n) memory).  Python integers: nothing overflows."""
    t, d, r = _survival_columns(time, event, risk)
    n = t.size
    order = np.argsort(t, kind="stable")
    t, d, r = t[order], d[order], r[order]
    later = np.searchsorted(t, t, side="right")                  # the first position with a later time
    ev = np.nonzero(d == 1.0)[0]
    comp = conc = disc = 0
    for lo in range(0, ev.size, int(chunk)):
        idx = ev[lo:lo + int(chunk)]
        start = later[idx]                                       # ascending, as idx is
        j0 = int(start[0])
        if j0 >= n:
            break
        valid = np.arange(j0, n)[None, :] >= start[:, None]
        ri, rj = r[idx][:, None], r[j0:][None, :]
        comp += int(valid.sum())
        conc += int(((ri > rj) & valid).sum())
        disc += int(((ri < rj) & valid).sum())
    return comp, conc, disc, comp - conc - disc


def cindex(counts: Sequence[int]) -> float:
    """C = (concordant + tied_risk / 2) / comparable from the four counts."""
    comp, conc, _, tied = (int(v) for v in counts)
    if comp <= 0:
        raise ValueError("no comparable pair: a concordance index needs an event followed by a later time")
    return (conc + 0.5 * tied) / comp


def concordance_index(time, event, risk) -> float:
    """Harrell's C of ``risk`` (higher = earlier event) against (time, event): ``cindex(concordance_counts(...))``."""
    return cindex(concordance_counts(time, event, risk))


def survival_summary(coef_tstr, coef_trtr, counts_tstr: Sequence[int], counts_trtr: Sequence[int],
                     event_shares: Mapping[str, float]) -> Dict[str, float]:
    """The ``survival_*`` keys from the fit trained on synthetic patients (TSTR) and the one trained on real ones (TRTR):
    ``coef_*`` their coefficient vectors in RAW-feature units (w * scale of the fit's own standardisation), ``counts_*`` the
    concordance counts of their risks on the real test cohort, ``event_shares`` the share of events per cohort name.  Keys:
    ``survival_tstr_cindex``, ``survival_trtr_cindex``, ``survival_cindex_gap`` (TRTR - TSTR), ``survival_coef_cosine`` (NaN when a
    fit is identically zero), ``survival_comparable_pairs`` and ``survival_event_share_<cohort>``."""
    a, b = np.asarray(coef_tstr, dtype=np.float64).ravel(), np.asarray(coef_trtr, dtype=np.float64).ravel()
    if a.shape != b.shape or a.size == 0:
        raise ValueError("the two coefficient vectors must have the same length")
    if int(counts_tstr[0]) != int(counts_trtr[0]):
        raise ValueError("both fits must be scored on the same test cohort")
    s, t = cindex(counts_tstr), cindex(counts_trtr)
    na, nb = float(np.sqrt(a @ a)), float(np.sqrt(b @ b))
    out = {"survival_tstr_cindex": float(s), "survival_trtr_cindex": float(t), "survival_cindex_gap": float(t - s),
           "survival_coef_cosine": float(a @ b) / (na * nb) if na > 0 and nb > 0 else float("nan"),
           "survival_comparable_pairs": float(int(counts_trtr[0]))}
    for name, share in event_shares.items():
        out[f"survival_event_share_{name}"] = float(share)
    return out
