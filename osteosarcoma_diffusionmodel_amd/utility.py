"""Downstream-utility metrics, host side: the L-BFGS driver that fits up to four regularised linear heads
through an ``eval_fn`` -- the device kernel behind ``DeviceKernels.glm_eval`` or a float64 restatement, the driver cannot tell --,
the exact rank-sum AUC, R^2, the propensity MSE, and the summaries that turn fits into the ``utility_*`` and ``c2st_*`` result keys
of ``BiologicalValidator.downstream_utility`` / ``discriminator_test``.  numpy float64 throughout; no device code: this module
imports on a machine without a GPU."""
from __future__ import annotations

from typing import Callable, Dict, Sequence, Tuple

import numpy as np

LOGISTIC, SQUARED = 0, 1          # OSD_GLM_LOGISTIC / OSD_GLM_SQUARED of include/osdiff.h
MAX_HEADS = 4                     # heads of one osd_val_glm_eval call


def _lbfgs(objective: Callable[[np.ndarray], Tuple[float, np.ndarray]], w: np.ndarray, max_iter: int, tol: float, history: int):
    """The L-BFGS loop ``fit_glm`` and ``survival.fit_cox`` share: minimises ``objective(w) -> (f, g)`` over a flat float64 vector
    from ``w`` -- two-loop recursion over ``history`` pairs, backtracking Armijo steps, the steepest descent when the quasi-Newton
    direction finds no step.  Returns ``(w, iterations, converged, |g|_inf)``; a line search that finds no step at all ends the loop
    with ``converged=False``."""
    f, g = objective(w)
    pairs = []                                                   # (s, y, 1 / y.s), oldest first
    it, converged = 0, bool(np.abs(g).max() <= tol)
    while not converged and it < max_iter:
        # two-loop recursion: d = -H g
        q = g.copy()
        alphas = []
        for s, y, rho in reversed(pairs):
            a = rho * float(s @ q)
            alphas.append(a)
            q -= a * y
        if pairs:
            s, y, _ = pairs[-1]
            q *= float(s @ y) / float(y @ y)
        for (s, y, rho), a in zip(pairs, reversed(alphas)):
            q += (a - rho * float(y @ q)) * s
        d = -q
        slope = float(g @ d)
        if not slope < 0.0:                                      # not a descent direction: forget the curvature
            pairs, d = [], -g
            slope = float(g @ d)
        step = 1.0 if pairs else 1.0 / max(1.0, float(np.abs(g).sum()))
        moved = False
        for attempt in range(2):                                 # the quasi-Newton direction, then the steepest descent
            t = step
            for _ in range(40):
                f_new, g_new = objective(w + t * d)
                if np.isfinite(f_new) and f_new <= f + 1e-4 * t * slope:
                    moved = True
                    break
                t *= 0.5
            if moved or not pairs:
                break
            pairs, d = [], -g
            slope = float(g @ d)
            step = 1.0 / max(1.0, float(np.abs(g).sum()))
        if not moved:
            break                                                # the noise floor of eval_fn: a clean end, not converged
        s_vec, y_vec = t * d, g_new - g
        sy = float(s_vec @ y_vec)
        if sy > 1e-12 * float(np.sqrt((s_vec @ s_vec) * (y_vec @ y_vec))):
            pairs.append((s_vec, y_vec, 1.0 / sy))
            if len(pairs) > history:
                pairs.pop(0)
        w, f, g = w + s_vec, f_new, g_new
        it += 1
        converged = bool(np.abs(g).max() <= tol)
    return w, it, converged, float(np.abs(g).max())


def fit_glm(eval_fn: Callable[[np.ndarray], Tuple[np.ndarray, np.ndarray]], K: int, D: int, kinds: Sequence[int], n: float, l2: float,
            max_iter: int = 200, tol: float = 1e-5, history: int = 10) -> Dict[str, object]:
    """Minimise  F(W) = sum_k [ loss_k(W) / n + (l2 / 2) |W_k[:D]|^2 ]  over W [K, D + 1] (bias last, unpenalised) by L-BFGS (two-loop
    recursion, ``history`` pairs) with backtracking Armijo steps, from W = 0.  ``eval_fn(W) -> (loss [K], grad [K, D + 1])`` returns
    SUMS over the rows, as ``osd_val_glm_eval`` does, and is all the driver knows about the data; ``n`` is the total row weight.  The
    heads are separable, so one joint vector serves them all.  ``kinds`` (LOGISTIC / SQUARED per head) is checked, not used: the
    link function lives in ``eval_fn``.

    Returns ``{"W", "iterations", "converged", "grad_inf_norm"}``: converged means the gradient's infinity norm fell to ``tol``.  A
    line search that finds no Armijo step even along the steepest descent -- an ``eval_fn`` in fp32 has reached its noise floor --
    ends the fit with ``converged=False``; nothing is raised."""
    K, D = int(K), int(D)
    kinds = [int(v) for v in kinds]
    if K < 1 or D < 1 or len(kinds) != K or any(v not in (LOGISTIC, SQUARED) for v in kinds):
        raise ValueError("fit_glm needs K >= 1 heads, D >= 1 features and one kind (LOGISTIC / SQUARED) per head")
    if not (n > 0 and l2 >= 0 and max_iter >= 0 and history >= 1):
        raise ValueError("fit_glm needs n > 0, l2 >= 0, max_iter >= 0 and history >= 1")
    n, l2 = float(n), float(l2)

    def objective(w):
        loss, grad = eval_fn(w.reshape(K, D + 1))
        loss = np.asarray(loss, dtype=np.float64).reshape(K)
        grad = np.asarray(grad, dtype=np.float64).reshape(K, D + 1)
        W = w.reshape(K, D + 1)
        f = float(loss.sum() / n + 0.5 * l2 * np.sum(W[:, :D] ** 2))
        g = grad / n
        g[:, :D] += l2 * W[:, :D]
        return f, g.ravel()

    w, it, converged, gnorm = _lbfgs(objective, np.zeros(K * (D + 1), dtype=np.float64), max_iter, tol, history)
    return {"W": w.reshape(K, D + 1).copy(), "iterations": it, "converged": converged, "grad_inf_norm": gnorm}


def roc_auc(scores, labels) -> float:
    """Area under the ROC curve in the rank-sum (Mann-Whitney) form with mid-ranks for ties: the share of (positive, negative) pairs
    the score orders correctly, a tie counting half.  Mid-ranks are multiples of 1/2, so every sum is exact in float64."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(labels).ravel()
    if s.shape != y.shape or s.size == 0:
        raise ValueError("roc_auc needs one label per score")
    pos = y > 0.5
    n_pos = int(pos.sum())
    n_neg = int(s.size - n_pos)
    if n_pos == 0 or n_neg == 0:
        raise ValueError("roc_auc needs both classes")
    _, inverse, counts = np.unique(s, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts).astype(np.float64)                  # rank of the last member of each tie group (1-based)
    mid = ends - (counts - 1) / 2.0
    rank_sum = float(mid[inverse.ravel()][pos].sum())
    return (rank_sum - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * n_neg)


def r2(pred, y) -> float:
    """Coefficient of determination 1 - sum (y - pred)^2 / sum (y - mean y)^2; NaN for a constant y."""
    p, t = np.asarray(pred, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    if p.shape != t.shape or t.size == 0:
        raise ValueError("r2 needs one prediction per target")
    tot = float(np.sum((t - t.mean()) ** 2))
    return 1.0 - float(np.sum((t - p) ** 2)) / tot if tot > 0 else float("nan")


def propensity_mse(p, c: float = 0.5) -> float:
    """Mean of (p - c)^2: how far a discriminator's propensities are from the share c of synthetic rows (0: indistinguishable;
    1/4 at c = 1/2 when every row is told apart with certainty)."""
    p = np.asarray(p, dtype=np.float64).ravel()
    if p.size == 0:
        raise ValueError("propensity_mse needs at least one propensity")
    return float(np.mean((p - float(c)) ** 2))


def sigmoid(z) -> np.ndarray:
    """1 / (1 + exp(-z)) without overflow."""
    z = np.asarray(z, dtype=np.float64)
    t = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def head_kinds(cond_blocks: Sequence[np.ndarray]) -> list:
    """One kind per condition column: LOGISTIC where every value of every block lies in {0, 1}, SQUARED otherwise."""
    blocks = [np.asarray(b, dtype=np.float64) for b in cond_blocks]
    K = blocks[0].shape[1]
    return [LOGISTIC if all(np.isin(b[:, k], (0.0, 1.0)).all() for b in blocks) else SQUARED for k in range(K)]


def utility_summary(names: Sequence[str], kinds: Sequence[int], tstr_scores, trtr_scores, y_tstr, y_trtr) -> Dict[str, float]:
    """The ``utility_*`` keys from the test cohort's scores [rows, K] under the fit trained on synthetic patients (TSTR) and under
    the fit trained on real ones (TRTR).  ``y_tstr`` / ``y_trtr``: the test targets [rows, K] as each fit saw its own -- 0/1 for a
    logistic head, standardised by the fit's training cohort for a squared one.  Per head ``utility_tstr_auc_<name>``,
    ``utility_trtr_auc_<name>`` and ``utility_auc_gap_<name>`` (TRTR - TSTR), or the same three with ``r2``; ``utility_gap_mean`` is the
    mean gap over the heads."""
    a, b = np.asarray(tstr_scores, dtype=np.float64), np.asarray(trtr_scores, dtype=np.float64)
    ya, yb = np.asarray(y_tstr, dtype=np.float64), np.asarray(y_trtr, dtype=np.float64)
    K = len(kinds)
    if len(names) != K or any(m.ndim != 2 or m.shape[1] != K for m in (a, b, ya, yb)):
        raise ValueError("one name, one kind and one score and target column per head")
    out, gaps = {}, []
    for k, (name, kind) in enumerate(zip(names, kinds)):
        if kind == LOGISTIC:
            tag, s, t = "auc", roc_auc(a[:, k], ya[:, k]), roc_auc(b[:, k], yb[:, k])
        else:
            tag, s, t = "r2", r2(a[:, k], ya[:, k]), r2(b[:, k], yb[:, k])
        out[f"utility_tstr_{tag}_{name}"] = float(s)
        out[f"utility_trtr_{tag}_{name}"] = float(t)
        out[f"utility_{tag}_gap_{name}"] = float(t - s)
        gaps.append(t - s)
    out["utility_gap_mean"] = float(np.mean(gaps))
    return out


def c2st_summary(z_real, z_synth) -> Dict[str, float]:
    """The ``c2st_*`` keys from the held-out logits of a real (label 0) against synthetic (label 1) discriminator: ``c2st_auc``,
    ``c2st_accuracy`` -- balanced: the mean of the two classes' accuracies at p = 1/2, a propensity of exactly 1/2 counting half, so
    unequal held-out cohorts still give 1/2 for a blind classifier -- and ``c2st_pmse``, the mean of (p - 1/2)^2 over the held-out
    rows.  0.5, 0.5 and 0 mean the cohorts are indistinguishable."""
    zr, zs = np.asarray(z_real, dtype=np.float64).ravel(), np.asarray(z_synth, dtype=np.float64).ravel()
    if zr.size == 0 or zs.size == 0:
        raise ValueError("a classifier two-sample test needs held-out rows of both cohorts")
    z = np.concatenate([zr, zs])
    y = np.concatenate([np.zeros(zr.size), np.ones(zs.size)])
    acc_r = float(np.mean((zr < 0) + 0.5 * (zr == 0)))
    acc_s = float(np.mean((zs > 0) + 0.5 * (zs == 0)))
    return {"c2st_auc": roc_auc(z, y), "c2st_accuracy": 0.5 * (acc_r + acc_s), "c2st_pmse": propensity_mse(sigmoid(z), 0.5)}


def split_indices(n: int, test_fraction: float, seed: int):
    """(train, test) index arrays of a seeded permutation of n rows, each sorted; at least one row on each side."""
    n = int(n)
    if n < 2:
        raise ValueError("a split needs at least 2 rows")
    if not 0.0 < test_fraction < 1.0:
        raise ValueError("test_fraction must lie in (0, 1)")
    n_test = min(max(int(round(n * test_fraction)), 1), n - 1)
    perm = np.random.default_rng(int(seed)).permutation(n)
    return np.sort(perm[n_test:]), np.sort(perm[:n_test])
