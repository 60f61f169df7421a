"""Shared pieces of the loss tests (test_loss_cpu.py, test_gpu_loss.py): the matrix test's input recipe, an fp64 oracle that turns one
forward graph into the loss and gradients of any (kind, delta, weight table), and the conditioning of injected noise around L1's kink."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as O
from helpers import block_widths, philox_keep_mask

GRAD_RTOL = 5e-5          # tests/test_gpu_train_matrix.py
LOSS_RTOL = 1e-5
P_DROP = 0.2
SEED = (5 << 33) + 977
L1_MARGIN = 1e-4          # ten times the 1e-5 * max|pred| the tolerances allow the prediction (max|pred| ~ 1 at these inputs)

_cache = {}


def inputs(dims, hidden, n, seed=17):
    """tests/test_gpu_train_matrix.py's recipe: weights with non-trivial GroupNorm affines, 0/1 mutation columns, host-drawn t / noise
    and injected keep-masks."""
    key = ("in", dims, tuple(hidden), n, seed)
    if key not in _cache:
        mut, expr, pw, cd = dims
        D = mut + expr + pw
        sd = O.init_state_dict(O.param_shapes(mut, expr, pw, cd, hidden, 128), seed=seed)
        gen = torch.Generator().manual_seed(seed + 1)
        for k in sd:
            if k.endswith((".1.weight", ".5.weight")):
                sd[k] = 1 + 0.2 * torch.randn(sd[k].shape, generator=gen)
            if k.endswith((".1.bias", ".5.bias")):
                sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
        x = torch.randn(n, D, generator=gen)
        x[:, :mut] = (x[:, :mut] > 0).float()
        cond = torch.randn(n, cd, generator=gen)
        t = torch.randint(0, 1000, (n,), generator=gen)
        noise = torch.randn(n, D, generator=gen)
        injected = [(torch.rand(n, w, generator=gen) >= P_DROP).float() for w in block_widths(hidden)]
        _cache[key] = (sd, x, cond, t, noise, injected)
    return _cache[key]


def philox_masks(hidden, n, roff=0):
    """The host restatement of the keep-masks the kernels draw from SEED."""
    return [torch.from_numpy(philox_keep_mask(SEED, n, w, b, P_DROP, roff)) for b, w in enumerate(block_widths(hidden))]


class Fp64Oracle:
    """One float64 forward graph of ``O.training_forward(..., return_loss=False)``; ``loss_and_grads`` applies torch's own
    F.mse_loss / F.l1_loss / F.huber_loss to it and back-propagates through the kept graph."""

    def __init__(self, sd, x0, cond, t, noise, hidden, masks=None, p=0.0, schedule="cosine", T=1000):
        self.bufs = {k: v.double() for k, v in O.schedule_buffers(schedule, T).items()}
        self.leaves = {k: v.detach().clone().requires_grad_(True) for k, v in O.to_dtype(sd, torch.float64).items()}
        self.t, self.noise, self.x0 = t, noise.double(), x0.double()
        self.masks = None if masks is None else [m.double() for m in masks]
        self.p = p if masks is not None else 0.0
        self.hidden = hidden
        self.cond = cond.double()
        self.pred = O.training_forward(self.leaves, self.bufs, self.x0, self.cond, t, self.noise, len(hidden), 128, self.masks, self.p,
                                       return_loss=False)

    def eps_loss(self, pred, kind, delta=1.0, weights=None):
        """loss = 1/(n D) sum_r w[t_r] sum_f rho(d_rf), rho from torch's own loss functions (reduction='none')."""
        fn = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=delta)}[kind]
        per = fn(pred, self.noise, reduction="none")
        if weights is not None:
            per = per * torch.as_tensor(weights).double()[self.t].view(-1, 1)
        return per.sum() / per.numel()

    def grads_of(self, loss_fn):
        """(loss, {name: gradient}) of ``loss_fn(pred)`` for any scalar function of the prediction."""
        pd = self.pred.detach().requires_grad_(True)
        loss = loss_fn(pd)
        (g_pred,) = torch.autograd.grad(loss, pd)
        g = torch.autograd.grad(self.pred, list(self.leaves.values()), grad_outputs=g_pred, retain_graph=True, allow_unused=True)
        return loss.item(), {k: (torch.zeros_like(v) if gk is None else gk) for (k, v), gk in zip(self.leaves.items(), g)}

    def loss_and_grads(self, kind, delta=1.0, weights=None):
        return self.grads_of(lambda pd: self.eps_loss(pd, kind, delta, weights))


def predict_fp64(sd, x0, cond, t, noise, hidden, masks=None, p=0.0):
    """The oracle's prediction for one injected noise, without a graph."""
    bufs = {k: v.double() for k, v in O.schedule_buffers("cosine", 1000).items()}
    with torch.no_grad():
        return O.training_forward(O.to_dtype(sd, torch.float64), bufs, x0.double(), cond.double(), t, noise.double(), len(hidden), 128,
                                  None if masks is None else [m.double() for m in masks], p if masks is not None else 0.0, return_loss=False)


def condition_l1_noise(pred_fn, noise, margin=L1_MARGIN, rounds=4):
    """Move injected noise off L1's kink.  sign(d), d = eps_hat - eps, jumps at 0, so one residual that fp32 puts on the other side of
    0 moves a gradient by 2/(n D): no tolerance survives that.  While any |d| < margin in float64, that element's noise moves by
    16 * margin away from the prediction (the prediction follows the noise through x_t, hence the rounds; at most ``rounds``).
    ``pred_fn(noise_fp32) -> float64 prediction``.  Returns (fp32 noise, elements inside the margin round by round -- last entry 0 on
    success); the noise stays fp32-representable, it is what the device is handed."""
    noise = noise.clone().float()
    counts = []
    for _ in range(rounds + 1):
        d = pred_fn(noise) - noise.double()
        inside = d.abs() < margin
        counts.append(int(inside.sum()))
        if counts[-1] == 0 or len(counts) > rounds:
            break
        away = torch.where(d >= 0, -1.0, 1.0).double() * (16.0 * margin)       # d grows in magnitude when eps moves against its sign
        noise = torch.where(inside, (noise.double() + away).float(), noise)
    return noise, counts


def check(loss, grads, ref_loss, ref_grads, D, grad_rtol=GRAD_RTOL, loss_rtol=LOSS_RTOL, show=None):
    """tests/test_gpu_train_matrix.py's comparisons: loss, every gradient tensor, and the tail columns / rows of input_proj's and
    output_proj's gradients, each against its own max.  Returns (worst error / tolerance ratio, failures)."""
    worst, bad = 0.0, []

    def one(what, a, b, rtol, atol=1e-9):
        nonlocal worst
        a = np.asarray(a, dtype=np.float64)
        b = np.asarray(b.detach().double().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float64)
        tol = atol + rtol * np.abs(b).max()
        err = np.abs(a - b).max() if np.isfinite(a).all() else np.inf
        worst = max(worst, err / tol)
        if show:
            print(f"  [{show}] {what}: max|d|={err:.3e} tol={tol:.3e} ratio={err / tol:.3f}")
        if not err <= tol:
            bad.append(f"{what}: max|d|={err:.3e} > tol={tol:.3e}")

    one("loss", loss, ref_loss, loss_rtol, 0.0)
    for k, g in grads.items():
        one(f"grad {k}", g.double().numpy(), ref_grads[k], grad_rtol)
    tail = D % 32 + 4
    one("grad input_proj.weight tail columns", grads["unet.input_proj.weight"][:, -tail:].double().numpy(),
        ref_grads["unet.input_proj.weight"][:, -tail:], grad_rtol)
    one("grad output_proj.weight tail rows", grads["unet.output_proj.weight"][-tail:].double().numpy(),
        ref_grads["unet.output_proj.weight"][-tail:], grad_rtol)
    one("grad output_proj.bias tail", grads["unet.output_proj.bias"][-tail:].double().numpy(), ref_grads["unet.output_proj.bias"][-tail:], grad_rtol)
    return worst, bad
