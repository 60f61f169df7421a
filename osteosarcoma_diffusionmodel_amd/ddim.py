"""Strided DDIM sampling (Song et al., 2021): the step plan that ``osd_sample_chain_steps`` runs.

A plan of S steps evaluates the denoiser at timesteps tau_0 < ... < tau_{S-1} = T - 1 and runs s = S-1 first, down to s = 0.
Step s goes from tau = tau_s to tau' = tau_{s-1} (abar' = 1 at s = 0) and, like every reverse step of the library, is one affine
update x' = A*x + B*eps + C*z:

    x0^ = (x - sqrt(1 - abar)*eps) / sqrt(abar),   x' = sqrt(abar')*x0^ + sqrt(1 - abar' - sigma^2)*eps + sigma*z
    sigma = eta * sqrt((1 - abar') / (1 - abar)) * sqrt(1 - abar / abar')
    =>  A = sqrt(abar' / abar),  B = sqrt(1 - abar' - sigma^2) - sqrt(abar')*sqrt(1 - abar) / sqrt(abar),  C = sigma

With eta = 1 and S = T this is the reference's DDPM chain; eta = 0 is deterministic after x_T.  Pure host code.

``ddim_x0_table`` is the second table of a chain that clips the predicted x0 (``osd_sample_chain_clipped``): the same step unfolded at
x0^, so that the clamp can sit between the two halves.

Both tables take ``prediction`` (objective.PREDICTION_TYPES): what the network's output ``out`` is.  Only x0^ = P*x + Q*out depends on
it -- epsilon: P = 1/sqrt(abar), Q = -sqrt(1 - abar)/sqrt(abar); v_prediction: P = a, Q = -b; sample: P = 0, Q = 1, with a, b the model's
fp32 ``sqrt_alphas_cumprod`` / ``sqrt_one_minus_alphas_cumprod`` buffers -- while E, F and C = sigma do not, so the folded row of the other
types is A = E*P + F, B = E*Q.  The default, "epsilon", keeps the expressions above and its arrays, bit for bit.

``dpmpp_2m_table`` is the plan of the second-order multistep solver DPM-Solver++(2M) (Lu et al., 2022; ``osd_sample_chain_multistep``):
the eta = 0 step of ``ddim_x0_table`` plus one term in the previous step's clipped x0^.  ``logsnr_timesteps`` spaces a plan uniformly in
the log-SNR instead of in t; it is a plan like any other, for either solver.

``edit_timesteps`` and ``ddim_inversion_table`` are the plans of an edit (``model.invert`` / ``model.edit``):
the levels a patient is noised to, and DDIM inversion -- the eta = 0 step run upwards -- as rows for ``osd_sample_chain_steps``.

``known_level_table`` is the second table of a chain around observed values (``osd_sample_chain_known``): the noise level each
step arrives at, at which the observations are put back.
"""
from __future__ import annotations

import math

import numpy as np


def ddim_timesteps(T: int, S: int) -> np.ndarray:
    """int32 [S]: tau_s = floor((s + 1) * T / S) - 1, strictly increasing, tau_{S-1} = T - 1 (S = T: tau_s = s)."""
    T, S = int(T), int(S)
    if not 1 <= S <= T:
        raise ValueError(f"num_inference_steps={S} outside [1, {T}]")
    s = np.arange(1, S + 1, dtype=np.int64)
    return (s * T // S - 1).astype(np.int32)


def _host32(b):
    if hasattr(b, "detach"):
        b = b.detach().cpu().float().numpy()
    return np.asarray(b, dtype=np.float32).reshape(-1)


def _x0_reading(prediction: str, abar: np.ndarray, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod):
    """float64 (P [T], Q [T]) of x0^ = P*x + Q*out for v_prediction / sample.  a and b are the model's fp32 buffers when given -- the
    values the training target was formed with: pass them --, else fp32 square roots of abar and 1 - abar, which equal those buffers up to
    the last bit of the host's sqrt."""
    if prediction == "sample":
        return np.zeros_like(abar), np.ones_like(abar)
    if prediction != "v_prediction":
        raise ValueError(f"prediction_type must be 'epsilon', 'v_prediction' or 'sample', got {prediction!r}")
    ab32 = abar.astype(np.float32)
    a = np.sqrt(ab32) if sqrt_alphas_cumprod is None else _host32(sqrt_alphas_cumprod)
    b = np.sqrt(np.float32(1.0) - ab32) if sqrt_one_minus_alphas_cumprod is None else _host32(sqrt_one_minus_alphas_cumprod)
    if a.shape != abar.shape or b.shape != abar.shape:
        raise ValueError("the schedule buffers differ in length")
    return a.astype(np.float64), -b.astype(np.float64)


def _unfolded(abar, tau, s, eta):
    """float64 (E, F, sigma) of step s: x' = E*x0^ + F*x + sigma*z (ddim_x0_table's expressions; row 0: E = 1, F = 0)."""
    a = abar[tau[s]]
    ap = abar[tau[s - 1]] if s > 0 else 1.0
    ratio = (1.0 - ap) / (1.0 - a) if a < 1.0 else 0.0
    sigma = eta * math.sqrt(ratio) * math.sqrt(max(1.0 - a / ap, 0.0))
    direction = math.sqrt(max(1.0 - ap - sigma * sigma, 0.0))
    f = direction / math.sqrt(1.0 - a) if a < 1.0 else 0.0
    if s == 0:
        return 1.0, 0.0, sigma
    return math.sqrt(ap) - f * math.sqrt(a), f, sigma


def ddim_step_table(alphas_cumprod, timesteps, eta: float, prediction: str = "epsilon", *, sqrt_alphas_cumprod=None,
                    sqrt_one_minus_alphas_cumprod=None):
    """(int32 [S] timesteps, fp32 [S][4] rows (A_s, B_s, C_s, 0)) for ``osd_sample_chain_steps``.

    ``prediction`` != "epsilon": A = E*P + F, B = E*Q of the unfolded step (module docstring), in float64, rounded once.

    The coefficients are formed in float64 from the fp32 ``alphas_cumprod`` buffer and rounded once to fp32, as
    ``osd_set_schedule`` folds the DDPM posterior.  The radicand of B is clamped at 0; x0^ is not clamped (as in the reference)."""
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"eta={eta} outside [0, 1]")
    if hasattr(alphas_cumprod, "detach"):
        alphas_cumprod = alphas_cumprod.detach().cpu().float().numpy()
    abar = np.asarray(alphas_cumprod, dtype=np.float32).astype(np.float64)
    tau = np.asarray(timesteps, dtype=np.int64).reshape(-1)
    T = abar.shape[0]
    if tau.size < 1 or tau.min() < 0 or tau.max() >= T:
        raise ValueError(f"timesteps must be a non-empty list inside [0, {T})")
    coef = np.zeros((tau.size, 4), dtype=np.float64)
    if prediction != "epsilon":
        P, Q = _x0_reading(prediction, abar, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod)
        for s in range(tau.size):
            e, f, sigma = _unfolded(abar, tau, s, eta)
            coef[s, :3] = (e * P[tau[s]] + f, e * Q[tau[s]], sigma)
        return tau.astype(np.int32), coef.astype(np.float32)
    for s in range(tau.size):
        a = abar[tau[s]]
        ap = abar[tau[s - 1]] if s > 0 else 1.0
        ratio = (1.0 - ap) / (1.0 - a) if a < 1.0 else 0.0
        sigma = eta * math.sqrt(ratio) * math.sqrt(max(1.0 - a / ap, 0.0))
        coef[s, 0] = math.sqrt(ap / a)
        coef[s, 1] = math.sqrt(max(1.0 - ap - sigma * sigma, 0.0)) - math.sqrt(ap) * math.sqrt(1.0 - a) / math.sqrt(a)
        coef[s, 2] = sigma
    return tau.astype(np.int32), coef.astype(np.float32)


def ddim_x0_table(alphas_cumprod, timesteps, eta: float, prediction: str = "epsilon", *, sqrt_alphas_cumprod=None,
                  sqrt_one_minus_alphas_cumprod=None) -> np.ndarray:
    """fp32 [S][4] rows (P_s, Q_s, E_s, F_s) for ``osd_sample_chain_clipped``: the step of ``ddim_step_table`` unfolded at x0^,

        x0^ = P*x + Q*eps,   x' = E*clip(x0^) + F*x + C*z       (C = sigma: slot 2 of ``ddim_step_table``'s row)
        P = 1/sqrt(abar),  Q = -sqrt(1 - abar)/sqrt(abar),  dir = sqrt(max(1 - abar' - sigma^2, 0))
        E = sqrt(abar') - dir*sqrt(abar)/sqrt(1 - abar),  F = dir/sqrt(1 - abar)

    so that the direction term uses the eps the clipped x0^ implies, (x - sqrt(abar)*x0c)/sqrt(1 - abar).  Without a clamp
    E*P + F = A and E*Q = B.  Formed in float64 from the fp32 buffer and rounded once, like ``ddim_step_table``, and rejecting what it
    rejects; row 0 has E = 1, F = 0 exactly (the last step returns the clipped x0^ itself).  ``prediction`` != "epsilon" changes (P, Q)
    only (module docstring); E and F keep their bits."""
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"eta={eta} outside [0, 1]")
    if hasattr(alphas_cumprod, "detach"):
        alphas_cumprod = alphas_cumprod.detach().cpu().float().numpy()
    abar = np.asarray(alphas_cumprod, dtype=np.float32).astype(np.float64)
    tau = np.asarray(timesteps, dtype=np.int64).reshape(-1)
    T = abar.shape[0]
    if tau.size < 1 or tau.min() < 0 or tau.max() >= T:
        raise ValueError(f"timesteps must be a non-empty list inside [0, {T})")
    coef = np.zeros((tau.size, 4), dtype=np.float64)
    for s in range(tau.size):
        a = abar[tau[s]]
        ap = abar[tau[s - 1]] if s > 0 else 1.0
        ratio = (1.0 - ap) / (1.0 - a) if a < 1.0 else 0.0
        sigma = eta * math.sqrt(ratio) * math.sqrt(max(1.0 - a / ap, 0.0))
        direction = math.sqrt(max(1.0 - ap - sigma * sigma, 0.0))
        f = direction / math.sqrt(1.0 - a) if a < 1.0 else 0.0
        coef[s] = (1.0 / math.sqrt(a), -math.sqrt(max(1.0 - a, 0.0)) / math.sqrt(a), math.sqrt(ap) - f * math.sqrt(a), f)
    coef[0, 2:] = (1.0, 0.0)
    if prediction != "epsilon":
        P, Q = _x0_reading(prediction, abar, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod)
        coef[:, 0], coef[:, 1] = P[tau], Q[tau]
    return coef.astype(np.float32)


def _logsnr(abar: np.ndarray) -> np.ndarray:
    """float64 lambda = ln(alpha / sigma) = (ln abar - ln(1 - abar)) / 2; +-inf where abar is 1 or 0."""
    with np.errstate(divide="ignore"):
        return 0.5 * (np.log(abar) - np.log1p(-abar))


def dpmpp_2m_table(alphas_cumprod, timesteps, prediction: str = "epsilon", *, sqrt_alphas_cumprod=None,
                   sqrt_one_minus_alphas_cumprod=None):
    """(int32 [S] timesteps, fp32 [S][4] rows (P_s, Q_s, G_s, F_s), fp32 [S] H_s) for ``osd_sample_chain_multistep``:

        x0^ = P*x + Q*out,   x' = G*clip(x0^) + F*x + H*clip(x0^)_prev       (prev: the step run before this one, s + 1)

    With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln(alpha / sigma), h_s = lambda' - lambda (' = at tau_{s-1}) and
    phi = -alpha' * expm1(-h_s):

        row S-1 (run first), and every row when S <= 2:   F = sigma'/sigma,  G = phi,               H = 0
        rows 0 < s < S-1:   r = (lambda_s - lambda_{s+1}) / h_s,   F = sigma'/sigma,  G = phi*(1 + 1/(2r)),  H = -phi/(2r)
        row 0 (the lower-order final step; h = inf):      F = 0,     G = 1,               H = 0     exactly

    G + H and F are ``ddim_x0_table(..., eta=0)``'s E and F up to fp32 rounding, so S <= 2 is DDIM at eta = 0; (P, Q) are that table's,
    bit for bit, for every ``prediction``.  Formed in float64 from the fp32 buffer and rounded once; rejects what the other tables
    reject, and a plan whose log-SNR does not strictly decrease along it."""
    pq = ddim_x0_table(alphas_cumprod, timesteps, 0.0, prediction, sqrt_alphas_cumprod=sqrt_alphas_cumprod,
                       sqrt_one_minus_alphas_cumprod=sqrt_one_minus_alphas_cumprod)
    abar = np.asarray(_host32(alphas_cumprod), dtype=np.float32).astype(np.float64)
    tau = np.asarray(timesteps, dtype=np.int64).reshape(-1)
    S = tau.size
    lam = _logsnr(abar[tau])
    if not np.isfinite(lam).all() or not (np.diff(lam) < 0).all():
        raise ValueError("the log-SNR must be finite and strictly decreasing along the plan")
    alpha, sigma = np.sqrt(abar[tau]), np.sqrt(1.0 - abar[tau])
    coef = np.zeros((S, 4), dtype=np.float64)
    hist = np.zeros(S, dtype=np.float64)
    coef[0, 2:] = (1.0, 0.0)
    for s in range(1, S):
        h = lam[s - 1] - lam[s]
        phi = -alpha[s - 1] * math.expm1(-h)
        coef[s, 2:] = (phi, sigma[s - 1] / sigma[s])
        if s < S - 1 and S > 2:
            r = (lam[s] - lam[s + 1]) / h
            coef[s, 2] = phi * (1.0 + 0.5 / r)
            hist[s] = -0.5 * phi / r
    out = coef.astype(np.float32)
    out[:, :2] = pq[:, :2]
    return tau.astype(np.int32), out, hist.astype(np.float32)


def logsnr_timesteps(alphas_cumprod, S: int) -> np.ndarray:
    """int32 [S]: a plan spaced uniformly in the log-SNR lambda = ln(sqrt(abar) / sqrt(1 - abar)), strictly increasing, tau_{S-1} = T - 1.

    S targets uniform in lambda between lambda(0) and lambda(T - 1), the nearest timestep for each, then made strictly increasing: an
    upward pass tau_i = max(tau_i, tau_{i-1} + 1), tau_{S-1} = T - 1, a downward pass tau_i = min(tau_i, tau_{i+1} - 1)."""
    abar = np.asarray(_host32(alphas_cumprod), dtype=np.float32).astype(np.float64)
    T, S = abar.shape[0], int(S)
    if not 1 <= S <= T:
        raise ValueError(f"num_inference_steps={S} outside [1, {T}]")
    lam = _logsnr(abar)
    if not np.isfinite(lam).all():
        raise ValueError("alphas_cumprod must lie strictly inside (0, 1)")
    targets = np.linspace(lam[0], lam[T - 1], S)
    tau = np.abs(lam[None, :] - targets[:, None]).argmin(axis=1).astype(np.int64)
    for i in range(1, S):
        tau[i] = max(tau[i], tau[i - 1] + 1)
    tau[S - 1] = T - 1
    for i in range(S - 2, -1, -1):
        tau[i] = min(tau[i], tau[i + 1] - 1)
    return tau.astype(np.int32)


def edit_timesteps(T: int, S: int, strength: float, alphas_cumprod=None, spacing: str = "uniform") -> np.ndarray:
    """int32 levels of an edit (``model.invert`` / ``model.edit``): the first K = max(1, round(strength * S)) timesteps of the S-step plan
    (``ddim_timesteps``, or ``logsnr_timesteps`` for ``spacing="logsnr"``, which needs ``alphas_cumprod``), with timestep 0 put in front
    when it is not there already, so that a replayed chain ends one tiny step above the clean patient.  Strictly increasing, K or K + 1
    entries; ``strength`` in (0, 1], and 1 gives the whole plan."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength={strength} outside (0, 1]")
    if spacing == "uniform":
        plan = ddim_timesteps(T, S)
    elif spacing == "logsnr":
        if alphas_cumprod is None:
            raise ValueError("spacing='logsnr' needs alphas_cumprod")
        if _host32(alphas_cumprod).shape[0] != int(T):
            raise ValueError(f"alphas_cumprod has {_host32(alphas_cumprod).shape[0]} entries, T is {int(T)}")
        plan = logsnr_timesteps(alphas_cumprod, S)
    else:
        raise ValueError(f"spacing must be 'uniform' or 'logsnr', got {spacing!r}")
    K = max(1, int(round(strength * int(S))))
    levels = plan[:K].astype(np.int32)
    if levels[0] != 0:
        levels = np.concatenate([np.zeros(1, dtype=np.int32), levels])
    return levels


def ddim_inversion_table(alphas_cumprod, levels, prediction: str = "epsilon", *, sqrt_alphas_cumprod=None,
                         sqrt_one_minus_alphas_cumprod=None):
    """(int32 [n] timesteps, fp32 [n][4] rows (A, B, 0, 0)), n = len(levels) - 1: DDIM inversion (Song et al. 2021, the deterministic
    encoder) as a plan for ``osd_sample_chain_steps`` -- the eta = 0 step run upwards.

    The patient is the state at ``levels[0]`` (pass it as ``x_T``), which must have b = sqrt(1 - abar) > 0; ``levels`` strictly increase.
    Step j evaluates the denoiser at the level the state is at, ``levels[j]``, and goes to ``levels[j + 1]`` (' = there):

        x0^ = P*x + Q*out,   F = b'/b,   E = a' - F*a,   x' = E*x0^ + F*x      =>   A = E*P + F,  B = E*Q,  C = 0

    with a = sqrt(abar), b = sqrt(1 - abar) and (P, Q) the reading of ``prediction`` (module docstring).  Float64 from the fp32 buffers,
    rounded once, like the other tables.  The rows come in the order the chain runs them, s = n - 1 first: row n - 1 - j is step j, so
    the first step run is the one at ``levels[0]`` and row 0 (C = 0, as every row) is the step that arrives at ``levels[-1]``."""
    abar = np.asarray(_host32(alphas_cumprod), dtype=np.float32).astype(np.float64)
    lv = np.asarray(levels, dtype=np.int64).reshape(-1)
    T = abar.shape[0]
    if lv.size < 2:
        raise ValueError("an inversion needs at least two levels: where the patient is and where the state goes")
    if lv.min() < 0 or lv.max() >= T or not (np.diff(lv) > 0).all():
        raise ValueError(f"levels must strictly increase inside [0, {T})")
    if not abar[lv[0]] < 1.0:
        raise ValueError(f"levels[0]={int(lv[0])} has abar = 1: the state there carries no noise to scale (b = 0)")
    if prediction == "epsilon":
        a0 = np.sqrt(abar)
        P, Q = 1.0 / a0, -np.sqrt(np.maximum(1.0 - abar, 0.0)) / a0
    else:
        P, Q = _x0_reading(prediction, abar, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod)
    n = lv.size - 1
    coef = np.zeros((n, 4), dtype=np.float64)
    for j in range(n):
        t, tn = lv[j], lv[j + 1]
        a, b = math.sqrt(abar[t]), math.sqrt(1.0 - abar[t])
        an, bn = math.sqrt(abar[tn]), math.sqrt(max(1.0 - abar[tn], 0.0))
        f = bn / b
        e = an - f * a
        coef[n - 1 - j, :2] = (e * P[t] + f, e * Q[t])
    return lv[:-1][::-1].astype(np.int32).copy(), coef.astype(np.float32)


def known_level_table(sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, timesteps) -> np.ndarray:
    """fp32 [S][2] rows (La_s, Ls_s) for ``osd_sample_chain_known``: the level step s arrives at, tau' = tau_{s-1}.

    Row s > 0 gathers (sqrt_alphas_cumprod[tau_{s-1}], sqrt_one_minus_alphas_cumprod[tau_{s-1}]) from the model's fp32 buffers --
    nothing is recomputed --, row 0 is (1, 0): the last step returns the observations themselves."""
    def host(b):
        if hasattr(b, "detach"):
            b = b.detach().cpu().float().numpy()
        return np.asarray(b, dtype=np.float32).reshape(-1)
    sa, s1 = host(sqrt_alphas_cumprod), host(sqrt_one_minus_alphas_cumprod)
    tau = np.asarray(timesteps, dtype=np.int64).reshape(-1)
    T = sa.shape[0]
    if s1.shape[0] != T:
        raise ValueError("the two schedule buffers differ in length")
    if tau.size < 1 or tau.min() < 0 or tau.max() >= T:
        raise ValueError(f"timesteps must be a non-empty list inside [0, {T})")
    level = np.empty((tau.size, 2), dtype=np.float32)
    level[0] = (1.0, 0.0)
    level[1:, 0] = sa[tau[:-1]]
    level[1:, 1] = s1[tau[:-1]]
    return level
