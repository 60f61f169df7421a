"""The training objective's options: what the network predicts, which loss the fused training step computes and how its rows are weighted.

Pure host code (like ``ddim.py``): the argument checks and the per-timestep weight tables.  The arithmetic itself runs in the
output_proj epilogue of ``osd_train_loss_fwd_bwd`` (csrc/epilogues.h: ``EpiLoss``, configured through ``osd_set_loss``).

With d = eps_hat - eps, row r at timestep t_r, n rows and D features::

    loss = 1/(n D) * sum_r w[t_r] * sum_f rho(d_rf)

    l2      rho = d^2                                                    F.mse_loss (the reference's loss and the default)
    l1      rho = |d|                                                    F.l1_loss
    huber   rho = d^2 / 2 if |d| <= delta else delta (|d| - delta / 2)     F.huber_loss(delta=delta)

``w`` is an optional table of T non-negative weights; without one every row weighs 1.  The mean is over n D and is NOT renormalised
by the sum of the weights: a table scales the loss (and the gradients) with it, as the usual min-SNR formulation does.

The reference declares ``model.diffusion.loss_type`` in its config.yaml and never reads it; here the key is honoured.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

LOSS_KINDS = {"l2": 0, "l1": 1, "huber": 2}         # include/osdiff.h: OSD_LOSS_*
LOSS_WEIGHTINGS = (None, "min_snr")
# what the network predicts (config['model']['diffusion']['prediction_type']; include/osdiff.h: OSD_PRED_*).  With a = sqrt(abar_t),
# b = sqrt(1 - abar_t): "epsilon" -- target eps, the reference's and the default --, "v_prediction" -- target a*eps - b*x0 (Salimans & Ho
# 2022) --, "sample" -- target x0.  The loss above then reads d = out - target
PREDICTION_TYPES = {"epsilon": 0, "v_prediction": 1, "sample": 2}


def check_prediction_type(prediction_type) -> str:
    if not isinstance(prediction_type, str) or prediction_type not in PREDICTION_TYPES:
        raise ValueError(f"prediction_type must be 'epsilon', 'v_prediction' or 'sample', got {prediction_type!r}")
    return prediction_type


# how the 0/1 mutation block of the output is read (config['model']['diffusion']['mutation_link']): "identity" --
# an unbounded x0^ like every other column, the default -- or "logistic" -- the logit of the Bernoulli mean E[x0 | x_t], trained by
# cross-entropy and sampled through sigma.  "logistic" needs prediction_type "sample": the linked columns are x0^
MUTATION_LINKS = ("identity", "logistic")


def check_mutation_link(mutation_link, prediction_type=None) -> str:
    if not isinstance(mutation_link, str) or mutation_link not in MUTATION_LINKS:
        raise ValueError(f"mutation_link must be 'identity' or 'logistic', got {mutation_link!r}")
    if mutation_link == "logistic" and prediction_type is not None and prediction_type != "sample":
        raise ValueError(f"mutation_link 'logistic' needs prediction_type 'sample' (the linked columns are x0^), "
                         f"but prediction_type is {prediction_type!r}")
    return mutation_link


def link_loss(out: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per-element cross-entropy of a logit against a target in [0, 1]: max(o, 0) - o y + log1p(exp(-|o|)), the form the training
    step's epilogue evaluates (``F.binary_cross_entropy_with_logits(reduction="none")``)."""
    return out.clamp_min(0) - out * target + torch.log1p(torch.exp(-out.abs()))


def check_loss_type(loss_type) -> str:
    if not isinstance(loss_type, str) or loss_type not in LOSS_KINDS:
        raise ValueError(f"loss_type must be 'l2', 'l1' or 'huber', got {loss_type!r}")
    return loss_type


def check_huber_delta(delta) -> float:
    try:
        d = float(delta)
    except (TypeError, ValueError):
        raise ValueError(f"huber_delta must be a positive finite number, got {delta!r}") from None
    if not (d > 0.0 and math.isfinite(d)):
        raise ValueError(f"huber_delta must be a positive finite number, got {delta!r}")
    return d


def check_loss_weighting(weighting) -> Optional[str]:
    if weighting in ("none", "None", ""):
        weighting = None
    if weighting not in LOSS_WEIGHTINGS:
        raise ValueError(f"loss_weighting must be None or 'min_snr', got {weighting!r}")
    return weighting


def check_gamma(gamma) -> float:
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"min_snr_gamma must be a positive finite number, got {gamma!r}") from None
    if not (g > 0.0 and math.isfinite(g)):
        raise ValueError(f"min_snr_gamma must be a positive finite number, got {gamma!r}")
    return g


def check_weight_table(weights, num_steps: int) -> np.ndarray:
    """A custom per-timestep table as a contiguous host float32 array of ``num_steps`` non-negative finite entries."""
    w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
    if w.ndim != 1 or w.shape[0] != num_steps:
        raise ValueError(f"loss weights must have shape [{num_steps}] (one per timestep), got {tuple(w.shape)}")
    w = np.ascontiguousarray(w, dtype=np.float32)
    if not np.isfinite(w).all():
        raise ValueError("loss weights must be finite")
    if (w < 0).any():
        raise ValueError("loss weights must be non-negative")
    return w


def min_snr_weights(alphas_cumprod, gamma: float = 5.0, prediction: str = "epsilon") -> torch.Tensor:
    """min-SNR-gamma weights (Hang et al. 2023): fp32 [T] with SNR_t = abar_t / (1 - abar_t), formed in float64 from the (fp32)
    ``alphas_cumprod`` buffer and rounded once.  The weight of the x0-loss is min(SNR_t, gamma); expressed on each type's own target:

        epsilon        w_t = min(SNR_t, gamma) / SNR_t          1 wherever SNR_t <= gamma (the noisy end), gamma / SNR_t towards t = 0
        v_prediction   w_t = min(SNR_t, gamma) / (SNR_t + 1)
        sample         w_t = min(SNR_t, gamma)"""
    g = check_gamma(gamma)
    prediction = check_prediction_type(prediction)
    ab = alphas_cumprod.detach().cpu() if isinstance(alphas_cumprod, torch.Tensor) else torch.as_tensor(np.asarray(alphas_cumprod))
    ab = ab.to(torch.float64).reshape(-1)
    if ab.numel() == 0 or not bool(((ab > 0) & (ab < 1)).all()):
        raise ValueError("alphas_cumprod must lie strictly inside (0, 1)")
    snr = ab / (1.0 - ab)
    if prediction == "epsilon":
        w = torch.clamp(snr, max=g) / snr
    elif prediction == "v_prediction":
        w = torch.clamp(snr, max=g) / (snr + 1.0)
    else:
        w = torch.clamp(snr, max=g)
    return w.to(torch.float32)


def loss_table(weighting: Optional[str], gamma: float, alphas_cumprod, custom: Optional[np.ndarray],
               prediction: str = "epsilon") -> Optional[np.ndarray]:
    """The table handed to ``osd_set_loss``: a custom one wins, then the configured weighting in the form of the model's prediction
    type, else None (every row weighs 1)."""
    if custom is not None:
        return custom
    if weighting == "min_snr":
        return np.ascontiguousarray(min_snr_weights(alphas_cumprod, gamma, prediction).numpy())
    return None
