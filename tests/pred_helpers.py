"""Float64 oracles of the prediction types (test_pred_cpu.py, test_gpu_pred.py): the training target and its loss on top of
loss_helpers.Fp64Oracle.grads_of, the three readings of a raw output, and the reverse chain unfolded at x0^ -- x0^ from (P, Q), then the
step's own expressions in x0^, x and z, which do not know what the network predicts.

a = sqrt_alphas_cumprod[t] and b = sqrt_one_minus_alphas_cumprod[t] are the model's fp32 buffers taken to float64: the values the
device's target is formed with."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as O
from helpers import FULL_H

PREDICTIONS = ("v_prediction", "sample")


def pq(prediction, a, b):
    """(P, Q) of x0^ = P x + Q out."""
    if prediction == "epsilon":
        return 1.0 / a, -b / a
    if prediction == "v_prediction":
        return a, -b
    if prediction == "sample":
        return torch.zeros_like(a), torch.ones_like(a)
    raise KeyError(prediction)


def target64(prediction, a, b, x0, noise):
    """The training target in float64; a, b broadcast against the rows."""
    return {"epsilon": noise, "v_prediction": a * noise - b * x0, "sample": x0}[prediction]


def readings(prediction, a, b, x, out):
    """{"x0", "eps", "v"} of a raw output: x0^ = P x + Q out, eps^ = (x - a x0^)/b, v^ = a eps^ - b x0^."""
    P, Q = pq(prediction, a, b)
    x0 = P * x + Q * out
    eps = (x - a * x0) / b
    return {"x0": x0, "eps": eps, "v": a * eps - b * x0}


def row_scalars(bufs, t):
    """(a, b) as [n, 1] float64 columns gathered by the rows' timesteps from schedule buffers (fp32 values)."""
    a = bufs["sqrt_alphas_cumprod"].float().double()[t].view(-1, 1)
    b = bufs["sqrt_one_minus_alphas_cumprod"].float().double()[t].view(-1, 1)
    return a, b


def min_snr64(alphas_cumprod, gamma, prediction):
    """The three min-SNR-gamma forms in float64 from the fp32 buffer."""
    ab = torch.as_tensor(alphas_cumprod).float().double()
    snr = ab / (1.0 - ab)
    m = torch.clamp(snr, max=gamma)
    return {"epsilon": m / snr, "v_prediction": m / (snr + 1.0), "sample": m}[prediction]


def loss_fn(orc, prediction, kind="l2", delta=1.0, weights=None, flip_b=False):
    """pred -> the scalar loss of loss_helpers.Fp64Oracle ``orc`` against the target of ``prediction``: torch's own loss functions,
    mean over n D, rows weighted by weights[t].  flip_b: the v target with the sign of b flipped (a negative control)."""
    a, b = row_scalars(O.schedule_buffers("cosine", 1000), orc.t)
    target = target64(prediction, a, -b if flip_b else b, orc.x0, orc.noise)
    fn = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": lambda p, q, reduction: F.huber_loss(p, q, reduction=reduction, delta=delta)}[kind]

    def loss(pred):
        per = fn(pred, target, reduction="none")
        if weights is not None:
            per = per * torch.as_tensor(weights).double()[orc.t].view(-1, 1)
        return per.sum() / per.numel()
    return loss


def model_sd64(m):
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.startswith(("condition_embed", "unet"))}
    return O.to_dtype(sd, torch.float64)


def guided_out(w, c0, space="raw", prediction="epsilon"):
    """out_fn of ``chain64``: classifier-free guidance combined on the raw output (space="raw": what the device does), or in eps-space --
    each branch converted to eps^, combined there, and converted back to the type's raw output (space="eps")."""
    def fn(sd, x, t_norm, cond, a, b):
        c0_rows = torch.as_tensor(c0, dtype=x.dtype).reshape(1, -1).repeat(x.shape[0], 1)
        out_c = O.unet_forward(sd, x, t_norm, O.condition_embed(sd, cond), len(FULL_H), 128, None, 0.0)
        out_u = O.unet_forward(sd, x, t_norm, O.condition_embed(sd, c0_rows), len(FULL_H), 128, None, 0.0)
        if space == "raw":
            return out_u + w * (out_c - out_u)
        e_c, e_u = readings(prediction, a, b, x, out_c)["eps"], readings(prediction, a, b, x, out_u)["eps"]
        eps = e_u + w * (e_c - e_u)
        # back to the raw output of the type: eps^ = Ue x + Ve out  =>  out = (eps^ - Ue x) / Ve
        P, Q = pq(prediction, a, b)
        return (eps - (1.0 - a * P) / b * x) / (-a * Q / b)
    return fn


def chain64(m, cond, x_start, z_of_s, taus, eta, prediction, *, sd=None, out_fn=None, known=None, lo=None, hi=None):
    """The reverse chain in float64, unfolded.  Per step, abar = alphas_cumprod[tau_s], abar' = alphas_cumprod[tau_{s-1}] (1 at s = 0):

        x0^ = P x + Q out                                   (P, Q) of ``prediction`` from the fp32 sqrt buffers; clamped to [lo, hi] if given
        taus given:  x' = sqrt(abar') x0^ + dir (x - sqrt(abar) x0^)/sqrt(1 - abar) + sigma z,
                     sigma = eta sqrt((1-abar')/(1-abar)) sqrt(1 - abar/abar'), dir = sqrt(max(1 - abar' - sigma^2, 0))
        taus None:   the DDPM posterior of every timestep: x' = (sqrt(abar') beta x0^ + sqrt(alpha) (1 - abar') x)/(1 - abar) + sqrt((1-abar')/(1-abar) beta) z,
                     the last step returns x0^

    known (NaN = free): observed elements are overwritten after every step with sqrt(abar') known + sqrt(1 - abar') z, at s = 0 with the
    observation.  out_fn(sd, x, t_norm, cond, a, b): another evaluation of the network (guidance)."""
    sd = model_sd64(m) if sd is None else sd
    Tm = m.num_steps
    abar = m.alphas_cumprod.detach().cpu().float().double()
    betas = m.betas.detach().cpu().float().double()
    sa = m.sqrt_alphas_cumprod.detach().cpu().float().double()
    sb = m.sqrt_one_minus_alphas_cumprod.detach().cpu().float().double()
    ddpm = taus is None
    if ddpm:
        taus = np.arange(Tm)
    cond = cond.detach().cpu().double()
    x = x_start.detach().cpu().double()
    c_emb = O.condition_embed(sd, cond)
    kn = obs = None
    if known is not None:
        kn = known.detach().cpu().double()
        obs = ~torch.isnan(kn)
    n_s = len(taus)
    one = torch.tensor(1.0, dtype=torch.float64)
    for s in reversed(range(n_s)):
        tau = int(taus[s])
        a, b = sa[tau], sb[tau]
        ab = abar[tau]
        abp = abar[int(taus[s - 1])] if s > 0 else one
        t_norm = torch.full((x.shape[0],), tau / Tm, dtype=torch.float64)
        out = O.unet_forward(sd, x, t_norm, c_emb, len(FULL_H), 128, None, 0.0) if out_fn is None else out_fn(sd, x, t_norm, cond, a, b)
        P, Q = pq(prediction, a, b)
        x0 = P * x + Q * out
        if lo is not None:
            x0 = torch.minimum(torch.maximum(x0, torch.as_tensor(lo).double()), torch.as_tensor(hi).double())
        z = z_of_s(s).detach().cpu().double() if (s > 0 and z_of_s is not None) else None
        if ddpm:
            if s > 0:
                nxt = (torch.sqrt(abp) * betas[tau] * x0 + torch.sqrt(1 - betas[tau]) * (1 - abp) * x) / (1 - ab)
                nxt = nxt + torch.sqrt((1 - abp) / (1 - ab) * betas[tau]) * z
            else:
                nxt = x0
        else:
            sigma = eta * torch.sqrt((1 - abp) / (1 - ab)) * torch.sqrt(1 - ab / abp)
            direction = torch.sqrt(torch.clamp(1 - abp - sigma ** 2, min=0.0))
            nxt = torch.sqrt(abp) * x0 + direction * (x - torch.sqrt(ab) * x0) / torch.sqrt(1 - ab)
            if s > 0 and float(sigma) != 0.0 and z is not None:
                nxt = nxt + sigma * z
        x = nxt
        if kn is not None:
            x = torch.where(obs, kn, x) if s == 0 else torch.where(obs, torch.sqrt(abp) * kn + torch.sqrt(1 - abp) * z, x)
    return x
