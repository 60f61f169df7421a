"""Shared pieces of the logistic-link tests (test_link_cpu.py, test_gpu_link.py): fp64 restatements of the link loss and of the link inside
the reverse chain, on top of loss_helpers.Fp64Oracle, pred_helpers.loss_fn / chain64 and mask_helpers.

    o = out, y = target (x0: the type is "sample"; inside [0, 1] after a mixup), M = mutation_dim
    f <  M:  rho = max(o, 0) - o y + log1p(exp(-|o|))         (F.binary_cross_entropy_with_logits, reduction="none")
    f >= M:  rho(o - y) of the configured loss_type           (pred_helpers.loss_fn's torch functions)
    loss = 1/(n D) sum_r w[t_r] sum_f m_rf rho_rf             m = observed (all ones without NaN)

Sampling: x0^ = sigma(out) on the columns f < M, out elsewhere, which for a "sample" model is an ``out_fn`` of chain64."""
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as O
from helpers import FULL_H
from loss_helpers import L1_MARGIN, Fp64Oracle
from mask_helpers import zero_fill
from pred_helpers import loss_fn


def link_loss_fn(orc, M, kind="l2", delta=1.0, weights=None, observed=None):
    """pred -> the scalar link loss of loss_helpers.Fp64Oracle ``orc`` (whose x0 is the zero-filled target): cross-entropy on the
    columns [0, M), pred_helpers.loss_fn's rho of ``kind`` elsewhere, rows weighted by weights[t], unobserved elements left out, mean
    over n D."""
    y = orc.x0
    n, D = y.shape
    cont = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": lambda p, q, reduction: F.huber_loss(p, q, reduction=reduction, delta=delta)}[kind]
    is_link = (torch.arange(D) < M).view(1, -1)

    def loss(pred):
        per = torch.where(is_link, F.binary_cross_entropy_with_logits(pred, y, reduction="none"), cont(pred, y, reduction="none"))
        if observed is not None:
            per = per * observed.double()
        if weights is not None:
            per = per * torch.as_tensor(weights).double()[orc.t].view(-1, 1)
        return per.sum() / per.numel()
    return loss


def identity_loss_fn(orc, kind="l2", delta=1.0, weights=None):
    """The same objective without a link: pred_helpers.loss_fn for the "sample" target."""
    return loss_fn(orc, "sample", kind, delta, weights)


class LinkOracle:
    """fp64 loss and gradients of the link objective for x0 with NaN = not observed (none: the plain objective)."""

    def __init__(self, sd, x0, cond, t, noise, hidden, M, masks=None, p=0.0):
        self.M = M
        self.observed = ~torch.isnan(x0)
        self.inner = Fp64Oracle(sd, zero_fill(x0), cond, t, noise, hidden, masks, p)

    @property
    def pred(self):
        return self.inner.pred

    def loss_and_grads(self, kind, delta=1.0, weights=None):
        return self.inner.grads_of(link_loss_fn(self.inner, self.M, kind, delta, weights, self.observed))


def condition_l1_x0_cont(pred_fn, x0, M, margin=L1_MARGIN, rounds=4):
    """mask_helpers.condition_l1_x0 on the continuous columns f >= M only: the link loss is smooth and needs none, and its 0 / 1 targets
    must stay 0 / 1.  Returns (fp32 x0 with its NaN, observed continuous elements inside the margin round by round)."""
    x0 = x0.clone().float()
    live = ~torch.isnan(x0)
    live[:, :M] = False
    counts = []
    for _ in range(rounds + 1):
        xf = zero_fill(x0)
        d = pred_fn(xf) - xf.double()
        inside = (d.abs() < margin) & live
        counts.append(int(inside.sum()))
        if counts[-1] == 0 or len(counts) > rounds:
            break
        away = torch.where(d >= 0, -1.0, 1.0).double() * (16.0 * margin)
        x0 = torch.where(inside, (xf.double() + away).float(), x0)
    return x0, counts


def link_columns(out, M):
    """sigma on the columns [0, M), the rest unchanged."""
    return torch.cat([torch.sigmoid(out[:, :M]), out[:, M:]], dim=1)


def link_out(M, inner=None):
    """out_fn of pred_helpers.chain64 for a linked "sample" model: the network's output (or ``inner``'s, e.g. pred_helpers.guided_out on
    the raw outputs -- guidance in logit space) with sigma on the columns [0, M)."""
    def fn(sd, x, t_norm, cond, a, b):
        if inner is None:
            out = O.unet_forward(sd, x, t_norm, O.condition_embed(sd, cond), len(FULL_H), 128, None, 0.0)
        else:
            out = inner(sd, x, t_norm, cond, a, b)
        return link_columns(out, M)
    return fn


def link_eps_fn(M):
    """The same as the eps_fn(sd, x, t_norm, cond) of test_solver_cpu.dpmpp_chain (prediction="sample")."""
    inner = link_out(M)
    return lambda sd, x, t_norm, cond: inner(sd, x, t_norm, cond, None, None)
