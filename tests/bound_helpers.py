"""Float64 reference of the per-patient variational bound (test_bound_cpu.py, test_gpu_bound.py), written from the formulas of
DESIGN.md section 3.18 and independent of osteosarcoma_diffusionmodel_amd/likelihood.py (which it does not import):

    se[r]  = sum_d (out[r][d] - target[r][d])^2           eval-mode network at q_sample(x0, t_r); target of the prediction type
    c_t    = sqrt(abar_{t-1}) beta_t / (1 - abar_t),  bt_t = (1 - abar_{t-1}) / (1 - abar_t) beta_t          (t >= 1)
    L_t    = c_t^2 / (2 bt_t) Q_t^2 se[t],   Q_t^2 = (1 - abar_t)/abar_t | 1 - abar_t | 1   (epsilon | v_prediction | sample)
    L_0    = D/2 ln(2 pi s2) + Q_0^2 se[0] / (2 s2),  s2 = betas[0] unless given
    L_T    = (abar |x0|^2 - D abar - D ln(1 - abar)) / 2,  abar = abar_{T-1}
    nll    = L_T + L_0 + (T - 1)/(S - 1) sum_{t in the sweep, t >= 1} L_t

The network is loss_helpers.Fp64Oracle's forward graph, the targets are pred_helpers.target64's; the schedule values are the fp32
buffers taken to float64, the values the device works from."""
import math

import numpy as np
import torch

from oracle import diffusion_oracle as O
from loss_helpers import Fp64Oracle, inputs
from pred_helpers import row_scalars, target64


def se64(sd, x0, cond, t, noise, hidden, prediction="epsilon", *, schedule="cosine", T=1000, masks=None, p=0.0):
    """Per-row ((pred - target)^2).sum(1) in float64 for rows (x0[r], cond[r], t[r], noise[r]).  masks / p: train-mode dropout
    (a negative control; the bound is an eval-mode quantity)."""
    orc = Fp64Oracle(sd, x0, cond, t, noise, hidden, masks, p, schedule, T)
    a, b = row_scalars(O.schedule_buffers(schedule, T), t)
    target = target64(prediction, a, b, x0.double(), noise.double())
    return ((orc.pred.detach() - target) ** 2).sum(1)


def sweep_se64(sd, x0, cond, timesteps, noise, hidden, prediction="epsilon", *, schedule="cosine", T=1000):
    """se [S][n] of every (timestep, patient) pair; noise [S][n][D]."""
    n = x0.shape[0]
    rows = []
    for s, t in enumerate(timesteps):
        rows.append(se64(sd, x0, cond, torch.full((n,), int(t), dtype=torch.int64), noise[s], hidden, prediction, schedule=schedule, T=T))
    return torch.stack(rows)


def q_sq64(abar, prediction):
    return {"epsilon": (1 - abar) / abar, "v_prediction": 1 - abar, "sample": torch.ones_like(abar)}[prediction]


def posterior64(bufs):
    """(c_t, bt_t) [T] in float64 with the expressions of O.posterior_coefficients (c_t = col 2 / col 3, bt_t = col 5 squared); entry 0
    is NaN: the reference's last step has no posterior."""
    betas, abar = bufs["betas"].float().double(), bufs["alphas_cumprod"].float().double()
    c = torch.full_like(abar, float("nan"))
    bt = torch.full_like(abar, float("nan"))
    c[1:] = torch.sqrt(abar[:-1]) * betas[1:] / (1 - abar[1:])
    bt[1:] = (1 - abar[:-1]) / (1 - abar[1:]) * betas[1:]
    return c, bt


def k64(bufs, prediction, q_of=None):
    """K_t = c_t^2 / (2 bt_t) Q_t^2 [T], entry 0 NaN.  q_of: the type whose Q_t^2 is used (a negative control)."""
    c, bt = posterior64(bufs)
    return c ** 2 / (2 * bt) * q_sq64(bufs["alphas_cumprod"].float().double(), q_of or prediction)


def bound64(se, timesteps, bufs, prediction, x0, *, decoder_variance=None, k_shift=0, q_of=None):
    """{"nll", "bpd", "prior", "terms"} in float64 from se [S][n] (timesteps ascending from 0).  k_shift: K taken from timestep
    t + k_shift (a negative control); q_of: see k64."""
    se = torch.as_tensor(se).double()
    ts = torch.as_tensor(np.asarray(timesteps), dtype=torch.int64)
    betas, abar = bufs["betas"].float().double(), bufs["alphas_cumprod"].float().double()
    T, D = betas.shape[0], x0.shape[1]
    assert int(ts[0]) == 0 and bool((ts[1:] > ts[:-1]).all())
    K = k64(bufs, prediction, q_of)
    s2 = float(betas[0]) if decoder_variance is None else float(decoder_variance)
    S = ts.numel()
    terms = torch.zeros_like(se)
    terms[0] = 0.5 * D * math.log(2 * math.pi * s2) + q_sq64(abar, q_of or prediction)[0] * se[0] / (2 * s2)
    if S > 1:
        idx = torch.clamp(ts[1:] + k_shift, 1, T - 1)
        terms[1:] = (T - 1) / (S - 1) * K[idx].view(-1, 1) * se[1:]
    a = float(abar[-1])
    prior = 0.5 * (a * (x0.double() ** 2).sum(1) - D * a - D * math.log(1 - a))
    nll = prior + terms.sum(0)
    return {"nll": nll, "bpd": nll / (D * math.log(2.0)), "prior": prior, "terms": terms}


def rows_missing(got, want, rtol):
    """Share of entries of ``got`` further than rtol * |want| from ``want``, entry by entry."""
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu() if isinstance(want, torch.Tensor) else want, dtype=np.float64)
    return float(np.mean(~(np.abs(got - want) <= rtol * np.abs(want))))


def auc_pairs(member, other):
    """Brute force: the share of (member, other) pairs with member < other, ties counting half."""
    wins = sum((a < b) + 0.5 * (a == b) for a in member for b in other)
    return wins / (len(member) * len(other))


# ---- the sweep case shared by test_bound_cpu.py (negative controls, oracle against oracle) and test_gpu_bound.py (the device) ----
NEG_DIMS, NEG_H, NEG_N, NEG_T = (16, 480, 16, 3), [256, 256, 512, 256], 37, 40
_sweeps = {}


def sweep_case(prediction):
    """(sd, x0, cond, noise [40][37][512], timesteps 0..39, se [40][37] float64, fp32 schedule buffers) of the complete sweep on a
    40-step cosine schedule; computed once per type and left unchanged."""
    if prediction not in _sweeps:
        sd, x, cond, _, _, _ = inputs(NEG_DIMS, NEG_H, NEG_N)
        noise = torch.randn(NEG_T, NEG_N, sum(NEG_DIMS[:3]), generator=torch.Generator().manual_seed(23))
        ts = np.arange(NEG_T)
        se = sweep_se64(sd, x, cond, ts, noise, NEG_H, prediction, T=NEG_T)
        _sweeps[prediction] = (sd, x, cond, noise, ts, se, O.schedule_buffers("cosine", NEG_T))
    return _sweeps[prediction]
