"""Survival utility, host side: the driver that fits an L2-regularised Cox proportional-hazards model
through an ``eval_fn`` -- the device kernels behind ``DeviceKernels.cox_eval`` or a float64 restatement, the driver cannot tell --,
Harrell's concordance as exact pair counts, and the summary that turns two fits and their counts into the ``survival_*`` result keys
of ``BiologicalValidator.survival_utility``; and, for ``prognostic_fidelity`` (section 3.32), the per-feature Newton driver
``univariate_cox`` and the screen ``cox_screen`` over ``DeviceKernels.cox_score``.  numpy float64 throughout; no device code: this
module imports on a machine without a GPU."""
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


# ---- the univariate Cox screen: one model per feature -----------------------------------------------------
def _two_sided_p(z: np.ndarray) -> np.ndarray:
    from scipy.special import ndtr
    return np.minimum(2.0 * ndtr(-np.abs(z)), 1.0)


def univariate_cox(eval_fn: Callable[[np.ndarray], Tuple[np.ndarray, np.ndarray, np.ndarray]], D: int, bound, max_iter: int = 15,
                   tol: float = 1e-8, max_abs_eta: float = 30.0, start=None) -> Dict[str, np.ndarray]:
    """D one-parameter Cox fits side by side, by Newton's method from beta = 0.  ``eval_fn(beta [D]) -> (loglik, score, info)``, float64
    [D] each, returns every column's partial log-likelihood, its derivative and minus its second derivative at that column's own
    beta, as ``osd_val_cox_score`` does, and is all the driver knows about the data.  ``bound`` [D]: R_c >= max_i |u_ic|.
    ``start``: the three arrays at beta = 0 where the caller has them already (a screen does), which saves that evaluation.

    One ``eval_fn`` call per iteration serves all columns.  A column proposes beta + step, step = score / info, clamped so that
    |beta_c| bound_c <= ``max_abs_eta`` (the exponent stays where exp holds it).  Where the log-likelihood did not fall the proposal is
    accepted and the next step comes from the new score and information; where it fell the column stays and its step is halved.  A
    column whose NEXT step, score / info at the beta it has just accepted (or at 0), is at most ``tol`` in size is converged and frozen
    there: that step is not taken.  A column that can no longer move because of the
    clamp (a feature that separates the events perfectly has no finite maximum) is frozen with ``converged=False`` and a finite
    beta at the clamp.  A column with info <= 0 or a non-finite value -- at 0: a constant feature, a cohort without events -- is marked
    ``failed``: beta, se, z and p are NaN.

    Returns float64 / bool / int64 [D] arrays: ``beta``, ``se`` = info^-1/2 at beta, ``z_wald`` = beta / se, ``p_wald`` (two-sided
    normal), ``loglik`` at beta, ``converged``, ``failed`` and ``iterations`` (the proposals a column made)."""
    D = int(D)
    if D < 1 or max_iter < 0 or not tol > 0 or not max_abs_eta > 0:
        raise ValueError("univariate_cox needs D >= 1, max_iter >= 0, tol > 0 and max_abs_eta > 0")
    R = np.asarray(bound, dtype=np.float64).reshape(D)
    if not (R >= 0).all():
        raise ValueError("bound must hold a non-negative number per column")
    with np.errstate(divide="ignore"):
        limit = np.where(R > 0, float(max_abs_eta) / np.where(R > 0, R, 1.0), np.inf)

    def evaluate(b, given=None):
        ll, sc, info = (np.asarray(v, dtype=np.float64).reshape(D) for v in (eval_fn(b) if given is None else given))
        return ll, sc, info, np.isfinite(ll) & np.isfinite(sc) & np.isfinite(info) & (info > 0)

    beta = np.zeros(D, dtype=np.float64)
    ll, sc, info, ok = evaluate(beta, start)
    ll, sc, info = ll.copy(), sc.copy(), info.copy()
    failed = ~ok
    converged = np.zeros(D, dtype=bool)
    iterations = np.zeros(D, dtype=np.int64)
    step = np.zeros(D, dtype=np.float64)
    step[ok] = sc[ok] / info[ok]
    converged[ok] = np.abs(step[ok]) <= tol                      # nothing to fit: the score is already zero
    active = ok & ~converged
    for _ in range(int(max_iter)):
        if not active.any():
            break
        cand = np.where(active, np.clip(beta + step, -limit, limit), beta)
        stuck = active & (cand == beta)                          # at the clamp and pushed further out
        active &= ~stuck
        if not active.any():
            break
        iterations[active] += 1
        ll2, sc2, info2, ok2 = evaluate(cand)
        broke = active & ~ok2
        failed |= broke
        active &= ~broke
        fell = active & (ll2 < ll - 1e-12 * (1.0 + np.abs(ll)))
        step[fell] *= 0.5
        take = active & ~fell
        beta[take], ll[take], sc[take], info[take] = cand[take], ll2[take], sc2[take], info2[take]
        step[take] = sc[take] / info[take]
        done = take & (np.abs(step) <= tol)
        converged |= done
        active &= ~done
    with np.errstate(divide="ignore", invalid="ignore"):
        se = np.where(failed, np.nan, 1.0 / np.sqrt(np.where(info > 0, info, np.nan)))
        out_beta = np.where(failed, np.nan, beta)
        z = out_beta / se
    return {"beta": out_beta, "se": se, "z_wald": z, "p_wald": np.where(failed, np.nan, _two_sided_p(np.nan_to_num(z))),
            "loglik": np.where(failed, np.nan, ll), "converged": converged & ~failed, "failed": failed, "iterations": iterations}


def cox_screen(k, x, plan, center, scale, mle: bool = True, max_iter: int = 15, tol: float = 1e-8) -> Dict[str, np.ndarray]:
    """The univariate Cox screen of one cohort: per feature of ``x`` [rows, D] (on ``k``'s device) the score test at beta = 0 and the
    hazard ratio per unit of u = (x - center) * scale.  ``k.cox_score(x, center, scale, plan, beta=None, bound=None, absmax=False)
    -> (loglik, score, info, absmax)`` is ``DeviceKernels.cox_score`` or a float64 stand-in; ``plan`` is ``k.cox_plan(time, event)``.

      ``z_score``, ``p_score``  score / sqrt(info) at 0 -- for a 0/1 feature its square is the log-rank chi-square -- and its two-sided
                                normal p-value
      ``q``                     ``diffexp.bh_qvalues`` over the features with a finite p; NaN elsewhere
      ``effect``                the log hazard ratio per unit of u: with ``mle`` the maximum-likelihood beta of ``univariate_cox``
                                (bound: the call's own max |u|), else the one-step estimate score / info at 0
      ``hr``                    exp(effect)
      ``score0``, ``info0``, ``absmax`` and, with ``mle``, every array of ``univariate_cox``

    A dropped feature (scale 0) has info 0: z, p, q and effect are NaN and ``failed`` is True."""
    from .diffexp import bh_qvalues
    D = int(x.shape[1])
    ll0, sc0, info0, absmax = k.cox_score(x, center, scale, plan, absmax=True)
    ll0, sc0, info0, absmax = (np.asarray(v, dtype=np.float64).reshape(D) for v in (ll0, sc0, info0, absmax))
    live = np.isfinite(sc0) & np.isfinite(info0) & (info0 > 0)
    safe = np.where(live, info0, 1.0)
    z = np.where(live, sc0 / np.sqrt(safe), np.nan)
    p = np.where(live, _two_sided_p(np.nan_to_num(z)), np.nan)
    q = np.full(D, np.nan)
    if live.any():
        q[live] = bh_qvalues(p[live])
    out = {"z_score": z, "p_score": p, "q": q, "score0": sc0, "info0": info0, "absmax": absmax}
    if mle:
        fit = univariate_cox(lambda b: k.cox_score(x, center, scale, plan, beta=b, bound=absmax)[:3], D, absmax, max_iter=max_iter,
                             tol=tol, start=(ll0, sc0, info0))
        out.update(fit)
        out["effect"] = fit["beta"]
    else:
        out["effect"] = np.where(live, sc0 / safe, np.nan)
        out["failed"], out["converged"] = ~live, live.copy()
    with np.errstate(over="ignore"):
        out["hr"] = np.exp(out["effect"])
    return out
