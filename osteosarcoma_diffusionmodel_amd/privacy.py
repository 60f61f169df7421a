"""Privacy accounting for differentially private training (``training.dp``): numpy only.

The mechanism of one DP-SGD step (Abadi et al. 2016) is the sampled Gaussian mechanism: a record joins the batch with probability
``q``, every record's gradient is clipped to norm C and N(0, sigma^2 C^2) noise is added to the sum.  Its Renyi divergence of order
alpha is (Mironov, Talwar, Zhang 2019, "Renyi Differential Privacy of the Sampled Gaussian Mechanism")

    eps_R(alpha) = log(A_alpha) / (alpha - 1),    A_alpha = E_{z ~ mu0} [(mu(z) / mu0(z))^alpha],
    mu0 = N(0, sigma^2),  mu = (1 - q) mu0 + q N(1, sigma^2),

which composes additively over steps and converts to (eps, delta) by eps = min_alpha T eps_R(alpha) + log(1 / delta) / (alpha - 1).
``log_moment`` evaluates log A_alpha -- a finite binomial sum at integer orders, the paper's two convergent series at fractional ones
--, ``epsilon`` minimises over a grid of both, ``noise_multiplier_for`` inverts it by bisection.

Two limits, stated wherever the number is shown: the account is for Poisson sampling at rate q = B / N while the loader shuffles
fixed-size batches (the usual approximation), and the library's noise generator is Philox, not a cryptographically secure one.
"""
from __future__ import annotations

import math

import numpy as np

# fractional orders resolve the optimum when it is small (large T, moderate sigma), integers up to 64 and a few powers of two beyond it
ORDERS = tuple([1.0 + x / 10.0 for x in range(1, 100)] + [float(a) for a in range(11, 64)] + [64.0, 96.0, 128.0, 192.0, 256.0, 384.0, 512.0, 1024.0])


def _log_add(a: float, b: float) -> float:
    """log(exp(a) + exp(b))"""
    if a == -np.inf:
        return b
    if b == -np.inf:
        return a
    hi, lo = max(a, b), min(a, b)
    return hi + math.log1p(math.exp(lo - hi))


def _log_sub(a: float, b: float) -> float:
    """log(exp(a) - exp(b)), a >= b"""
    if b == -np.inf:
        return a
    if a == b:
        return -np.inf
    if a < b:
        raise ValueError("log of a negative number")
    return a + math.log1p(-math.exp(b - a))


def _log_erfc(x: float) -> float:
    """log(erfc(x)); the asymptotic series where erfc underflows"""
    v = math.erfc(x)
    if v > 1e-300:
        return math.log(v)
    # erfc(x) ~ exp(-x^2) / (x sqrt(pi)) * (1 - 1/(2 x^2) + 3/(4 x^4) - 15/(8 x^6))
    return -x * x - math.log(x) - 0.5 * math.log(math.pi) + math.log1p(-0.5 / x ** 2 + 0.75 / x ** 4 - 1.875 / x ** 6)


def _log_a_int(q: float, sigma: float, alpha: int) -> float:
    """A_alpha = sum_k C(alpha, k) (1 - q)^(alpha - k) q^k exp((k^2 - k) / (2 sigma^2))"""
    k = np.arange(alpha + 1, dtype=np.float64)
    log_comb = np.concatenate([[0.0], np.cumsum(np.log((alpha - k[1:] + 1.0) / k[1:]))])
    terms = log_comb + k * math.log(q) + (alpha - k) * math.log1p(-q) + (k * k - k) / (2.0 * sigma ** 2)
    hi = float(terms.max())
    return hi + math.log(float(np.exp(terms - hi).sum()))


def _log_a_frac(q: float, sigma: float, alpha: float) -> float:
    """The two series of section 3.3 of the paper (z0 splits the real line where mu0 = mu's other component)."""
    log_a0, log_a1 = -np.inf, -np.inf
    z0 = sigma ** 2 * math.log(1.0 / q - 1.0) + 0.5
    i, coef = 0, 1.0          # coef = C(alpha, i) for real alpha, signed: alpha (alpha - 1) ... (alpha - i + 1) / i!
    while True:
        log_coef = math.log(abs(coef)) if coef != 0.0 else -np.inf
        j = alpha - i
        log_t0 = log_coef + i * math.log(q) + j * math.log1p(-q)
        log_t1 = log_coef + j * math.log(q) + i * math.log1p(-q)
        log_e0 = math.log(0.5) + _log_erfc((i - z0) / (math.sqrt(2.0) * sigma))
        log_e1 = math.log(0.5) + _log_erfc((z0 - j) / (math.sqrt(2.0) * sigma))
        log_s0 = log_t0 + (i * i - i) / (2.0 * sigma ** 2) + log_e0
        log_s1 = log_t1 + (j * j - j) / (2.0 * sigma ** 2) + log_e1
        if coef > 0:
            log_a0, log_a1 = _log_add(log_a0, log_s0), _log_add(log_a1, log_s1)
        elif coef < 0:
            log_a0, log_a1 = _log_sub(log_a0, log_s0), _log_sub(log_a1, log_s1)
        coef *= (alpha - i) / (i + 1.0)
        i += 1
        if max(log_s0, log_s1) < -30.0:          # A_alpha >= 1: terms below e^-30 are below 1e-13 of it
            break
        if i > 10000:
            raise RuntimeError("the fractional-order series did not converge")
    return _log_add(log_a0, log_a1)


def log_moment(q: float, noise_multiplier: float, alpha: float) -> float:
    """log A_alpha = log E_{z ~ mu0}[(mu / mu0)^alpha] of the sampled Gaussian mechanism, alpha > 1."""
    q, sigma, alpha = float(q), float(noise_multiplier), float(alpha)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"sample rate q={q} outside [0, 1]")
    if not alpha > 1.0:
        raise ValueError(f"order alpha={alpha} must exceed 1")
    if q == 0.0:
        return 0.0
    if sigma <= 0.0:
        return np.inf
    if q == 1.0:
        return alpha * (alpha - 1.0) / (2.0 * sigma ** 2)       # the plain Gaussian mechanism: eps_R = alpha / (2 sigma^2), exactly
    if alpha == math.floor(alpha):
        return _log_a_int(q, sigma, int(alpha))
    return _log_a_frac(q, sigma, alpha)


def rdp(q: float, noise_multiplier: float, steps: int, orders=ORDERS) -> np.ndarray:
    """Renyi divergence of ``steps`` compositions at every order."""
    return np.array([steps * log_moment(q, noise_multiplier, a) / (a - 1.0) for a in orders], dtype=np.float64)


def epsilon(q: float, noise_multiplier: float, steps: int, delta: float, orders=ORDERS) -> float:
    """The epsilon of (epsilon, delta)-DP spent by ``steps`` steps at sample rate ``q`` and noise multiplier sigma."""
    if not 0.0 < delta < 1.0:
        raise ValueError(f"delta={delta} outside (0, 1)")
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if steps == 0 or q == 0.0:
        return 0.0
    if noise_multiplier <= 0.0:
        return float("inf")
    r = rdp(q, noise_multiplier, steps, orders)
    a = np.asarray(orders, dtype=np.float64)
    return float(np.min(r + math.log(1.0 / delta) / (a - 1.0)))


def noise_multiplier_for(target_epsilon: float, q: float, steps: int, delta: float, orders=ORDERS, rtol: float = 1e-3) -> float:
    """The smallest sigma (to ``rtol``) whose ``epsilon(q, sigma, steps, delta)`` does not exceed ``target_epsilon``: bisection on the
    decreasing function sigma -> epsilon."""
    if not target_epsilon > 0.0:
        raise ValueError(f"target_epsilon={target_epsilon} must be positive")
    lo, hi = 0.0, 1.0
    while epsilon(q, hi, steps, delta, orders) > target_epsilon:
        lo, hi = hi, hi * 2.0
        if hi > 1e6:
            raise ValueError(f"no noise multiplier below 1e6 reaches epsilon={target_epsilon}")
    while hi - lo > rtol * hi:
        mid = 0.5 * (lo + hi)
        if epsilon(q, mid, steps, delta, orders) > target_epsilon:
            lo = mid
        else:
            hi = mid
    return hi


def check_dp_config(dp, training_config: dict, *, is_vae: bool = False, constraints: bool = False, world: int = 1):
    """Validate ``training.dp`` without touching a device.  Returns None when absent, else a dict with ``max_grad_norm``,
    ``noise_multiplier`` (None while only ``target_epsilon`` is known: it needs the planned number of steps), ``target_epsilon``,
    ``delta`` and ``seed``."""
    if dp is None:
        return None
    if not isinstance(dp, dict):
        raise ValueError("training.dp must be a mapping {max_grad_norm, noise_multiplier | target_epsilon, delta, seed}")
    unknown = set(dp) - {"max_grad_norm", "noise_multiplier", "target_epsilon", "delta", "seed"}
    if unknown:
        raise ValueError(f"training.dp: unknown keys {sorted(unknown)}")
    if "max_grad_norm" not in dp:
        raise ValueError("training.dp needs max_grad_norm (the per-patient gradient bound C)")
    c = float(dp["max_grad_norm"])
    if not (c > 0.0 and math.isfinite(c)):
        raise ValueError(f"training.dp.max_grad_norm={c} must be positive and finite")
    sigma, target = dp.get("noise_multiplier"), dp.get("target_epsilon")
    if (sigma is None) == (target is None):
        raise ValueError("training.dp needs exactly one of noise_multiplier and target_epsilon")
    if sigma is not None:
        sigma = float(sigma)
        if not (sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError(f"training.dp.noise_multiplier={sigma} must be >= 0 (0: clipping only, epsilon = inf)")
    if target is not None:
        target = float(target)
        if not (target > 0.0 and math.isfinite(target)):
            raise ValueError(f"training.dp.target_epsilon={target} must be positive and finite")
    delta = float(dp.get("delta", 1e-5))
    if not 0.0 < delta < 1.0:
        raise ValueError(f"training.dp.delta={delta} outside (0, 1)")
    seed = dp.get("seed")
    if seed is not None and not 0 <= int(seed) < 2 ** 64:
        raise ValueError("training.dp.seed must fit 64 bits")
    if float(training_config.get("augmentation", {}).get("mixup_alpha", 0.0)) > 0.0:
        raise ValueError("training.dp does not go with mixup (one record would reach two rows): set training.augmentation.mixup_alpha "
                         "to 0 -- the reference's default is 0.2")
    if constraints:
        raise ValueError("training.dp does not go with the constraint losses: they are batch statistics, a patient has no gradient of "
                         "their own (model.set_constraints() clears them)")
    if is_vae:
        raise ValueError("training.dp is not accepted for a cVAE model: its BatchNorm1d couples the rows of a batch")
    if world > 1:
        raise ValueError("training.dp runs on one process: data parallel is not supported")
    return {"max_grad_norm": c, "noise_multiplier": sigma, "target_epsilon": target, "delta": delta,
            "seed": None if seed is None else int(seed)}
