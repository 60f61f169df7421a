"""Shared by test_edit_cpu.py and test_gpu_edit.py: the noise map (osd_noise_map) and the DDIM inversion restated in NumPy / float64
torch, straight from their definitions (include/osdiff.h, ddim.py)."""
import numpy as np
import torch


def noise_map_definition(x0, eps, a, b, taus, coef, denoiser):
    """The definition of osd_noise_map, in the dtype of its inputs: x0 [n, D], eps [S, n, D], a / b the schedule buffers [T], taus [S],
    coef [S, 4] = (A, B, C, 0), denoiser(y, s) -> out.  Returns (y [S, n, D], cz [S-1, n, D] in the chain's draw order: cz[S-1-s] =
    C_s z_s = y_{s-1} - (A_s y_s + B_s out_s), outs [S, n, D] (outs[0] is None-free: evaluated too))."""
    S = len(taus)
    y = [a[taus[s]] * x0 + b[taus[s]] * eps[s] for s in range(S)]
    outs = [denoiser(y[s], s) for s in range(S)]
    cz = [None] * (S - 1)
    for s in range(1, S):
        cz[S - 1 - s] = y[s - 1] - (coef[s, 0] * y[s] + coef[s, 1] * outs[s])
    return y, cz, outs


def replay(x_start, cz, coef, denoiser, first_row=None):
    """The chain over the plan from x_start with C_s z_s = cz[S-1-s] added at step s; row 0 is ``first_row`` (A, B) when given.  Returns
    every state, states[s] being the one the step at level s returned (states[S] = x_start)."""
    S = coef.shape[0]
    x = x_start
    states = [None] * S + [x_start]
    for s in reversed(range(S)):
        A, B = (coef[s, 0], coef[s, 1]) if (s > 0 or first_row is None) else first_row
        x = A * x + B * denoiser(x, s)
        if s > 0:
            x = x + cz[S - 1 - s]
        states[s] = x
    return states


def oracle_denoiser(O, sd, cond, taus, T, n_hidden, dtype=torch.float64):
    """denoiser(y, s) over the oracle's network in ``dtype``: y a torch tensor [n, D] on the host."""
    sd = O.to_dtype(sd, dtype)
    c_emb = O.condition_embed(sd, cond.detach().cpu().to(dtype))

    def run(y, s):
        t_norm = torch.full((y.shape[0],), int(taus[s]) / T, dtype=dtype)
        return O.unet_forward(sd, y.to(dtype), t_norm, c_emb, n_hidden, 128, None, 0.0)
    return run


def ddim_inversion_oracle(abar, levels, x, denoiser, prediction="epsilon", a32=None, b32=None):
    """DDIM inversion in float64, unfolded: at levels[j], x0^ and eps^ from the output by the model's reading, then
    x' = sqrt(abar') x0^ + sqrt(1 - abar') eps^ at levels[j + 1].  denoiser(x, j) evaluates at levels[j]."""
    for j in range(len(levels) - 1):
        t, tn = int(levels[j]), int(levels[j + 1])
        a, b = torch.sqrt(abar[t]), torch.sqrt(1 - abar[t])
        out = denoiser(x, j)
        if prediction == "epsilon":
            x0 = (x - b * out) / a
        elif prediction == "sample":
            x0 = out
        else:
            x0 = a32[t] * x - b32[t] * out
        eps = (x - a * x0) / b
        x = torch.sqrt(abar[tn]) * x0 + torch.sqrt(1 - abar[tn]) * eps
    return x


def schedule(kind, T):
    """fp32 (alphas_cumprod, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod) with the model's expressions."""
    if kind == "linear":
        betas = torch.linspace(1e-4, 0.02, T)
    else:
        steps = torch.arange(T + 1, dtype=torch.float32) / T
        ab = torch.cos((steps + 0.008) / 1.008 * np.pi / 2) ** 2
        ab = ab / ab[0]
        betas = torch.clip(1 - (ab[1:] / ab[:-1]), 0.0001, 0.9999)
    abar = torch.cumprod(1.0 - betas, dim=0)
    return abar.numpy(), torch.sqrt(abar).numpy(), torch.sqrt(1.0 - abar).numpy()
