"""Shared pieces of the cVAE layer-op tests (test_nn_ops_cpu.py, test_gpu_nn_ops.py): the float64 references of the ops behind
``csrc/nn_ops.hip`` and the inputs the GPU tests feed them.  CPU only; plain torch in float64 with autograd, no hand-written gradient.

Stated fp32 tolerances (the docstrings of test_gpu_cvae.py and test_gpu_ops.py): outputs and losses 1e-5 * max|ref|; gradients
5e-5 * max|ref| + 3e-6; running statistics 1e-6 relative; a seeded dropout mask is exact.

The ReLU gate.  The device decides ``pre > 0`` on an fp32 pre-activation; an element within rounding of zero may gate the other way than
in float64, and one flipped gate moves sum(g) and sum(g zhat) of its whole column.  No test may depend on such an element, and no
column is dropped after the fact.  So the inputs are built to keep every live pre-activation at least MARGIN from zero:

  supplied mask   mask = 0 wherever |pre64| < MARGIN, on top of the random drops: y and every gradient are then independent of the gate
                  there on both sides.  At most FORCED_CAP of the elements may be forced (unit-scale data: about 2 * MARGIN * pdf(0)
                  ~ 0.008 %).
  no / seeded     small shapes only, with a hard-coded seed whose float64 min|pre| >= MARGIN (CHECKED_SEED).
  eval mode       the statistics do not depend on z: every z with |pre64| < MARGIN is moved so that pre = +-NUDGE.
  use_bn = 0      the gate is z > 0 on the same fp32 number on both sides: nothing to do.

test_nn_ops_cpu.py asserts these conditions for every seed and shape the GPU file uses."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import philox_keep_mask, philox_normals

OUT_RTOL, GRAD_RTOL, GRAD_ATOL, STAT_RTOL = 1e-5, 5e-5, 3e-6, 1e-6
MARGIN, NUDGE, FORCED_CAP = 1e-4, 1e-3, 1e-3
P_DROP, MOMENTUM, BN_EPS = 0.2, 0.1, 1e-5
TAG_USER = 0x55535200
LATENT_TAG = TAG_USER + 0x7E          # k_reparam's stream of seeded latent noise

# ---- shapes ------------------------------------------------------------------------------------------------------------------------
# (n, K1, K2, N) and where launch.h sends it.  Forward: A = w (lda = K1+K2), B0 = x1 (ldb0 = K1), F = N, K = K1+K2, K0 = K1.
#   glds_ok       needs K % 32 == 0 (no zero-padded A here), lda % 4 == ldb0 % 4 == 0 and, with a second panel, K1 % 32 == 0, K2 % 4 == 0
#   gemm_fast_ok  needs lda, ldb0, K multiples of 4 and, with a second panel, K1 % 32 == 0, K2 % 4 == 0, K2 >= 4
#   EpiBias::fast_ok needs N % 4 == 0 (and aligned bias / out): without it either kernel falls back to the guarded one
LINEAR_SHAPES = [
    ((2, 40, 3, 32), "anchor-two-panel-guarded(lda=43)"),
    ((5, 37, 3, 8), "K1%4!=0-concatenated-then-FAST-one-panel(K=40);dw+37-unaligned"),
    ((9, 37, 0, 5), "one-panel-guarded(K,N%4!=0)"),
    ((257, 64, 4, 130), "two-panel-guarded(K=68-passes-gemm_fast_ok,N=130%4!=0-fails-EpiBias::fast_ok)"),
    ((257, 64, 4, 132), "two-panel-FAST(K=68%32!=0:no-glds;K1%32==0,K2=4,N%4==0)"),
    ((130, 64, 32, 64), "two-panel-LDS-DMA(K=96%32==0,K1%32==0,K2%4==0,N%4==0)"),
    ((300, 128, 0, 1), "survival-head(N=1:guarded;fwd-K=128)"),
    ((1, 16, 3, 24), "single-row-two-panel-guarded(lda=19)"),
    ((64, 2000, 4, 256), "config1-first-layer-cond4-two-panel-guarded(K1=2000%32!=0)"),
]

BLOCK_MASKED_SHAPES = [(2, 1), (5, 63), (256, 64), (257, 65), (1030, 130), (4099, 257)]    # the last: 1 053 443 elements > 4096 * 256
BLOCK_P0_SHAPES = [(2, 1), (5, 63), (257, 65)]
BLOCK_EVAL_SHAPES = [(1, 7), (257, 65), (4099, 257)]
BLOCK_NOBN_SHAPES = [(300, 128), (3, 5)]
SEEDED_DROPOUT_SHAPES = [(257, 65), (5, 63), (1030, 130)]
CHECKED_SEED = {(2, 1): 0, (5, 63): 0, (257, 65): 3}     # float64 min|pre| >= MARGIN there (asserted in test_nn_ops_cpu.py)
MASKED_SEED = 11
REPARAM_SHAPES = [(1, 1), (3, 5), (7, 130), (4099, 257)]
REPARAM_SEEDED_SHAPES = [(3, 5), (257, 130)]
REPARAM_EXTREME_SHAPE = (64, 16)
VAE_LOSS_SHAPES = [(2, 1, 1), (3, 5, 7), (131, 2003, 16), (2050, 130, 129)]
MSE_COUNTS = [1, 63, 64, 65, 257, 262145]

# Worst per-element relative error of torch's own fp32 autograd d_logvar on the extreme-range inputs (reparam_extreme_inputs) against
# float64, as test_nn_ops_cpu.py measures and prints it.  The device kernel is held to REPARAM_EXTREME_FACTOR times this: its expf and
# its products may each be an ulp or two away from torch's.
REPARAM_EXTREME_FP32_ERR = 1.3e-7
REPARAM_EXTREME_FACTOR = 8.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def skewed(g, *shape):
    """Asymmetric random data with a non-zero mean (about 0.32; the squared-uniform part skews it)."""
    return 0.7 * torch.randn(*shape, generator=g) + 0.5 * torch.rand(*shape, generator=g) ** 2 + 0.15


# ---- Linear ------------------------------------------------------------------------------------------------------------------------
def linear_inputs(n, K1, K2, N):
    g = gen(1000 + n + 3 * K1 + 7 * K2 + 11 * N)
    x1 = skewed(g, n, K1)
    x2 = skewed(g, n, K2) if K2 else None
    w = torch.randn(N, K1 + K2, generator=g) / (K1 + K2) ** 0.5
    b = skewed(g, N)
    gy = skewed(g, n, N)
    return x1, x2, w, b, gy


def linear_ref(x1, x2, w, b, gy):
    """y, dx1, dw, db of F.linear(cat([x1, x2]), w, b) in float64 (x2 gets no gradient)."""
    x1d, wd, bd = (t.double().requires_grad_(True) for t in (x1, w, b))
    x = x1d if x2 is None else torch.cat([x1d, x2.double()], dim=1)
    y = F.linear(x, wd, bd)
    dx1, dw, db = torch.autograd.grad(y, [x1d, wd, bd], gy.double())
    return y.detach(), dx1, dw, db


# ---- BatchNorm1d -> ReLU -> Dropout ------------------------------------------------------------------------------------------------
def block_params(n, C, seed):
    """z, gamma, beta from one generator in that order (the order the seeds of CHECKED_SEED were checked with), then the running
    statistics, the upstream gradient and the uniform numbers of a random keep-mask."""
    g = gen(seed)
    z = 1.5 * torch.randn(n, C, generator=g) + 0.7
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    rm = 0.3 * torch.randn(C, generator=g)
    rv = 0.5 + torch.rand(C, generator=g)
    gy = skewed(g, n, C)
    u = torch.rand(n, C, generator=g)
    return dict(z=z, gamma=gamma, beta=beta, rm=rm, rv=rv, gy=gy, u=u)


def pre64(z, gamma, beta, rm, rv, training, eps=BN_EPS):
    """The float64 pre-activation BatchNorm hands the ReLU (running statistics untouched)."""
    return F.batch_norm(z.double(), rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), bool(training), 0.0, eps)


def forced_mask(u, pre, p=P_DROP):
    """0/1 keep-mask: the random drops (u < p) plus every element whose |pre| < MARGIN.  Returns (mask, number forced)."""
    near = pre.abs() < MARGIN
    return ((u >= p) & ~near).float(), int(near.sum())


def nudge_eval(z, gamma, beta, rm, rv, eps=BN_EPS):
    """Eval mode: move every z whose |pre| < MARGIN to where pre = +-NUDGE (the sign it had; + at exactly 0)."""
    pre = pre64(z, gamma, beta, rm, rv, False, eps)
    near = pre.abs() < MARGIN
    want = torch.where(pre >= 0, NUDGE, -NUDGE).double()
    std = torch.sqrt(rv.double() + eps)
    moved = rm.double() + (want - beta.double()) / gamma.double() * std
    return torch.where(near, moved, z.double()).float(), int(near.sum())


def stress_columns(z):
    """(257, 65) extras: column 3 constant (variance 0: save_invstd must be eps^-1/2), column 7 with mean 30 and std 0.03 (its
    E[z^2] - mean^2 loses seven digits: right in double, garbage if the column sums are ever narrowed to float)."""
    z = z.clone()
    z[:, 3] = 0.7
    z[:, 7] = 30.0 + 0.03 * (z[:, 7] - 0.7) / 1.5
    return z


def masked_case(n, C, seed=MASKED_SEED, stress=False):
    """Training + BN + supplied mask: the inputs, the mask with its forced drops, and their count."""
    c = block_params(n, C, seed)
    if stress:
        c["z"] = stress_columns(c["z"])
    c["mask"], c["forced"] = forced_mask(c.pop("u"), pre64(c["z"], c["gamma"], c["beta"], c["rm"], c["rv"], True))
    return c


def p0_case(n, C):
    c = block_params(n, C, CHECKED_SEED[(n, C)])
    c.pop("u")
    c["mask"] = None
    return c


def eval_case(n, C, seed=MASKED_SEED):
    c = block_params(n, C, seed)
    c.pop("u")
    c["z"], c["nudged"] = nudge_eval(c["z"], c["gamma"], c["beta"], c["rm"], c["rv"])
    c["mask"] = None
    return c


def nobn_case(n, C, seed=MASKED_SEED):
    c = block_params(n, C, seed)
    c["mask"] = (c.pop("u") >= P_DROP).float()
    return c


def block_ref(z, gy, gamma=None, beta=None, rm=None, rv=None, training=True, mask=None, p=0.0, momentum=MOMENTUM, eps=BN_EPS):
    """float64 F.batch_norm -> relu -> * mask / (1 - p) with autograd.  Returns a dict: y, dz and, with BatchNorm, dgamma, dbeta,
    save_mean, save_invstd and the running statistics F.batch_norm leaves behind."""
    out = {}
    zd = z.double().requires_grad_(True)
    if gamma is not None:
        gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        rm2, rv2 = rm.double().clone(), rv.double().clone()
        pre = F.batch_norm(zd, rm2, rv2, gd, bd, bool(training), momentum, eps)
        out["running_mean"], out["running_var"] = rm2, rv2
        if training:
            out["save_mean"] = z.double().mean(0)
            out["save_invstd"] = 1.0 / torch.sqrt(z.double().var(0, unbiased=False) + eps)
        else:
            out["save_mean"] = rm.double()
            out["save_invstd"] = 1.0 / torch.sqrt(rv.double() + eps)
    else:
        pre = zd
    y = F.relu(pre)
    if mask is not None and training:
        y = y * mask.double() / (1.0 - p)
    if gamma is not None:
        out["dz"], out["dgamma"], out["dbeta"] = torch.autograd.grad(y, [zd, gd, bd], gy.double())
    else:
        out["dz"], = torch.autograd.grad(y, [zd], gy.double())
    out["y"] = y.detach()
    return out


def keep_mask(seed, n, C, tag, p):
    """The device's seeded dropout mask (helpers.philox_keep_mask: block = the op's ``tag``)."""
    return torch.from_numpy(philox_keep_mask(seed, n, C, tag, p))


# ---- reparameterisation ------------------------------------------------------------------------------------------------------------
def reparam_inputs(n, Lz, seed=21):
    g = gen(seed + n + Lz)
    mu = torch.randn(n, Lz, generator=g) + 0.2
    lv = 0.5 * torch.randn(n, Lz, generator=g) - 0.3
    eps = torch.randn(n, Lz, generator=g)
    gz = skewed(g, n, Lz)
    return mu, lv, eps, gz


def reparam_extreme_inputs():
    """A trained, tight posterior far from the origin: mu ~ 30 randn, logvar ~ -12 + randn (std ~ 2.5e-3)."""
    n, Lz = REPARAM_EXTREME_SHAPE
    g = gen(5)
    mu = 30.0 * torch.randn(n, Lz, generator=g)
    lv = -12.0 + torch.randn(n, Lz, generator=g)
    eps = torch.randn(n, Lz, generator=g)
    gz = skewed(g, n, Lz)
    return mu, lv, eps, gz


def reparam_ref(mu, lv, eps, gz=None, dtype=torch.float64):
    """z = mu + eps exp(0.5 lv) in ``dtype`` and, with gz, (d_mu, d_logvar) by autograd."""
    m, l = (t.detach().to(dtype).clone().requires_grad_(True) for t in (mu, lv))
    z = m + eps.to(dtype) * torch.exp(0.5 * l)
    if gz is None:
        return z.detach()
    dmu, dlv = torch.autograd.grad(z, [m, l], gz.to(dtype))
    return z.detach(), dmu, dlv


def worst_rel(got, ref):
    """Worst element of |got - ref| / |ref| (float64)."""
    got, ref = torch.as_tensor(got).detach().double(), torch.as_tensor(ref).detach().double()
    return float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())


def reparam_extreme_fp32_err():
    """Worst-element relative error of torch's fp32 autograd d_logvar on reparam_extreme_inputs against float64."""
    mu, lv, eps, gz = reparam_extreme_inputs()
    return worst_rel(reparam_ref(mu, lv, eps, gz, torch.float32)[2], reparam_ref(mu, lv, eps, gz)[2])


def latent_noise(seed, n, Lz):
    return philox_normals(seed, n, Lz, 0, LATENT_TAG)


# ---- losses ------------------------------------------------------------------------------------------------------------------------
def vae_loss_inputs(n, D, Lz):
    g = gen(300 + n + D + Lz)
    x = skewed(g, n, D)
    xr = x + 0.5 * skewed(g, n, D)
    mu = torch.randn(n, Lz, generator=g) + 0.2
    lv = 0.5 * torch.randn(n, Lz, generator=g) - 0.3
    return xr, x, mu, lv


def vae_loss_ref(xr, x, mu, lv):
    """(total, recon, kl) as k_vae_loss documents them and the gradients of the total, float64:
    recon = sum (xr - x)^2 / n, kl = -0.5 sum(1 + lv - mu^2 - e^lv) / n."""
    xrd, md, ld = (t.double().requires_grad_(True) for t in (xr, mu, lv))
    n = x.shape[0]
    recon = ((xrd - x.double()) ** 2).sum() / n
    kl = -0.5 * (1 + ld - md ** 2 - ld.exp()).sum() / n
    total = recon + kl
    d_recon, d_mu, d_lv = torch.autograd.grad(total, [xrd, md, ld])
    return (total.item(), recon.item(), kl.item()), d_recon, d_mu, d_lv


def kl_atol(mu, lv):
    """0.5 * Lz * 2^-22 * max(1, max e^lv, max mu^2): see test_gpu_nn_ops.test_vae_loss."""
    Lz = mu.shape[1]
    big = max(1.0, float(lv.double().exp().max()), float((mu.double() ** 2).max()))
    return 0.5 * Lz * 2.0 ** -22 * big


def mse_inputs(count):
    g = gen(400 + count)
    a = skewed(g, count)
    b = a + 0.5 * skewed(g, count)
    return a, b


def mse_ref(a, b):
    ad = a.double().requires_grad_(True)
    loss = F.mse_loss(ad, b.double())
    da, = torch.autograd.grad(loss, [ad])
    return loss.item(), da
