"""The per-patient variational bound of the DDPM (Ho et al. 2020, eq. 5) and what is built on it.

    -log p(x0 | c)  <=  L_T + sum_{t >= 1} L_t + L_0          (nats)

The coefficients are those of the reference's ``p_sample`` (models/diffusion.py:401-419), read from the model's fp32 buffers ``betas``
and ``alphas_cumprod`` and promoted to float64.  With abar_t = alphas_cumprod[t], for t >= 1:

    c_t  = sqrt(abar_{t-1}) beta_t / (1 - abar_t)           the weight of x0^ in the posterior mean
    bt_t = (1 - abar_{t-1}) / (1 - abar_t) beta_t           the posterior variance
    L_t  = c_t^2 / (2 bt_t) |x0 - x0^|^2 = K_t se[t],       se = |out - target|^2, x0 - x0^ = -Q_t (out - target)
    K_t  = abar_{t-1} beta_t / (2 (1 - abar_t)(1 - abar_{t-1})) Q_t^2

Q_t^2 is (1 - abar_t)/abar_t for an epsilon model, 1 - abar_t for v_prediction, 1 for sample; K_t is formed as ONE float64 expression
per type, so no 1/abar_t (4e9 at the noisy end of the cosine schedule) appears as an intermediate.  L_t equals
(SNR_{t-1} - SNR_t)/2 |x0 - x0^|^2 only up to the fp32 rounding of the two buffers (6e-4 relative on the cosine schedule); the beta_t
form above is the definition.

The reference's last step is deterministic, so a density needs a decoder: L_0 = D/2 ln(2 pi s2) + Q_0^2 se[0] / (2 s2) with
s2 = ``decoder_variance``, by default betas[0] -- a convention, not something the reference fixes.  The prior term is
L_T = (abar |x0|^2 - D abar - D ln(1 - abar)) / 2 with abar = abar_{T-1}.

A subset of S timesteps -- t = 0 plus S - 1 timesteps strided over 1..T-1 -- estimates the sum:
L_T + L_0 + (T - 1)/(S - 1) sum_{t in subset, t >= 1} L_t.

Everything here is host arithmetic on small arrays; the T-fold forward sweep that produces ``se`` is the library's
(``osd_bound_sweep``: csrc/train.hip, the row-loss epilogue EpiRowSq in csrc/epilogues.h).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

PREDICTION_TYPES = ("epsilon", "v_prediction", "sample")


def _f64(v) -> np.ndarray:
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v).astype(np.float64)


def q_squared(alphas_cumprod, prediction_type: str) -> np.ndarray:
    """Q_t^2 [T] of x0 - x0^ = -Q_t (out - target), float64."""
    abar = _f64(alphas_cumprod)
    if prediction_type == "epsilon":
        return (1.0 - abar) / abar
    if prediction_type == "v_prediction":
        return 1.0 - abar
    if prediction_type == "sample":
        return np.ones_like(abar)
    raise ValueError(f"prediction_type must be one of {PREDICTION_TYPES}, got {prediction_type!r}")


def kl_weights(betas, alphas_cumprod, prediction_type: str) -> np.ndarray:
    """K_t [T] in float64 with L_t = K_t se[t] for t >= 1; entry 0 is 0 (t = 0 is the decoder term, ``assemble``)."""
    beta, abar = _f64(betas), _f64(alphas_cumprod)
    if beta.shape != abar.shape or beta.ndim != 1:
        raise ValueError("betas and alphas_cumprod must be vectors of the same length")
    k = np.zeros_like(abar)
    b, a, ap = beta[1:], abar[1:], abar[:-1]
    if prediction_type == "epsilon":
        k[1:] = ap * b / (2.0 * a * (1.0 - ap))
    elif prediction_type == "v_prediction":
        k[1:] = ap * b / (2.0 * (1.0 - ap))
    elif prediction_type == "sample":
        k[1:] = ap * b / (2.0 * (1.0 - a) * (1.0 - ap))
    else:
        raise ValueError(f"prediction_type must be one of {PREDICTION_TYPES}, got {prediction_type!r}")
    return k


def select_timesteps(T: int, num_timesteps: Optional[int] = None, timesteps: Optional[Sequence[int]] = None) -> np.ndarray:
    """The sweep's timesteps, ascending, 0 first.  Default: all T.  ``num_timesteps=S``: 0 plus S - 1 timesteps strided over
    1..T-1.  ``timesteps``: an explicit set; it must contain 0, lie in [0, T) and may not repeat."""
    if timesteps is not None:
        if num_timesteps is not None:
            raise ValueError("give num_timesteps or timesteps, not both")
        ts = np.asarray(list(timesteps))
        if ts.ndim != 1 or ts.size == 0 or not np.issubdtype(ts.dtype, np.integer):
            raise ValueError("timesteps must be a non-empty list of integers")
        if ts.min() < 0 or ts.max() >= T:
            raise ValueError(f"timesteps must lie in [0, {T})")
        if np.unique(ts).size != ts.size:
            raise ValueError("timesteps may not repeat")
        if 0 not in ts:
            raise ValueError("timesteps must contain 0 (the decoder term)")
        return np.sort(ts).astype(np.int32)
    if num_timesteps is None or int(num_timesteps) >= T:
        return np.arange(T, dtype=np.int32)
    S = int(num_timesteps)
    if S < 1:
        raise ValueError(f"num_timesteps must be >= 1, got {num_timesteps}")
    if S == 1:
        return np.zeros(1, dtype=np.int32)
    rest = np.unique(np.round(np.linspace(1, T - 1, S - 1)).astype(np.int64))
    return np.concatenate([[0], rest]).astype(np.int32)


def prior_term_np(x0_sq_norm, abar_last: float, D: int) -> np.ndarray:
    """L_T from |x0|^2 per row (float64)."""
    a = float(abar_last)
    return 0.5 * (a * _f64(x0_sq_norm) - D * a - D * math.log1p(-a))


def term_weights(timesteps, betas, alphas_cumprod, prediction_type: str, D: int, decoder_variance: Optional[float] = None):
    """(w [S], c0, scale) in float64 for a sweep over ``timesteps`` (ascending, 0 first): terms[s] = w[s] * se[s], plus c0 on row 0.
    Row 0 is the decoder term (w = Q_0^2 / (2 s2), c0 = D/2 ln(2 pi s2)); the others are scale * K_t with scale = (T - 1)/(S - 1), the
    weight a subset's L_t stand in with (1 for a complete sweep)."""
    ts = np.asarray(timesteps, dtype=np.int64)
    T = _f64(betas).shape[0]
    if ts.ndim != 1 or ts.size == 0 or ts[0] != 0 or np.any(np.diff(ts) <= 0) or ts[-1] >= T:
        raise ValueError("timesteps must ascend from 0 and stay below T")
    s2 = float(_f64(betas)[0]) if decoder_variance is None else float(decoder_variance)
    if not (s2 > 0.0 and math.isfinite(s2)):
        raise ValueError(f"decoder_variance must be positive and finite, got {decoder_variance}")
    n_rest = ts.size - 1
    scale = (T - 1) / n_rest if n_rest > 0 else 0.0
    w = kl_weights(betas, alphas_cumprod, prediction_type)[ts] * scale
    w[0] = q_squared(alphas_cumprod, prediction_type)[0] / (2.0 * s2)
    return w, 0.5 * D * math.log(2.0 * math.pi * s2), scale


def assemble(se, timesteps, betas, alphas_cumprod, prediction_type: str, prior, D: int, decoder_variance: Optional[float] = None) -> dict:
    """The bound on the host from the sweep's raw ``se`` [S][n] (any float type), the sweep's ``timesteps`` and the prior term [n]:
    float64 numpy arrays ``nll`` [n] (nats), ``bpd`` [n], ``terms`` [S][n] (row 0: L_0, the others scale * L_t, so that
    nll = prior + terms.sum(0)) and ``scale`` (``term_weights``)."""
    se = _f64(se)
    w, c0, scale = term_weights(timesteps, betas, alphas_cumprod, prediction_type, D, decoder_variance)
    if se.ndim != 2 or se.shape[0] != w.size:
        raise ValueError("se must be [S][n] with one row per timestep")
    terms = w[:, None] * se
    terms[0] += c0
    nll = _f64(prior) + terms[0] + terms[1:].sum(axis=0)
    return {"nll": nll, "bpd": nll / (D * math.log(2.0)), "terms": terms, "scale": scale}


# ---- membership inference on per-record scores (lower = "member") ----------------------------------------------------------
def auc_by_ranks(member_scores, other_scores) -> float:
    """P(member < other) + P(tie)/2: the Mann-Whitney statistic from midranks, on the host."""
    a, b = _f64(member_scores).ravel(), _f64(other_scores).ravel()
    if a.size == 0 or b.size == 0:
        raise ValueError("both cohorts need at least one score")
    allv = np.concatenate([a, b])
    order = np.argsort(allv, kind="mergesort")
    sv = allv[order]
    ranks = np.empty(allv.size, dtype=np.float64)
    i = 0
    while i < sv.size:
        j = i
        while j + 1 < sv.size and sv[j + 1] == sv[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    u_b = ranks[a.size:].sum() - b.size * (b.size + 1) / 2.0      # pairs in which the other cohort's score is the larger one (ties half)
    return float(u_b / (a.size * b.size))


def membership_metrics(member_scores, other_scores) -> dict:
    """``auc``, ``tpr_at_1pct_fpr`` and ``advantage`` (max over thresholds of TPR - FPR) of the attack "score <= threshold means member"."""
    a, b = _f64(member_scores).ravel(), _f64(other_scores).ravel()
    auc = auc_by_ranks(a, b)
    thr = np.unique(np.concatenate([a, b]))
    tpr = np.searchsorted(np.sort(a), thr, side="right") / a.size
    fpr = np.searchsorted(np.sort(b), thr, side="right") / b.size
    ok = fpr <= 0.01
    return {"auc": auc, "tpr_at_1pct_fpr": float(tpr[ok].max()) if ok.any() else 0.0, "advantage": float(max((tpr - fpr).max(), 0.0))}
