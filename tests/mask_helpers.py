"""Shared pieces of the masked-loss tests (test_mask_cpu.py, test_gpu_mask.py): the deterministic missing-value pattern, and an fp64 oracle
of the NaN-masked training loss on top of loss_helpers.Fp64Oracle.

    m = ~isnan(x0),  x~0 = where(m, x0, 0),  x_t = a x~0 + b eps,  target = eps | a eps - b x~0 | x~0
    loss = 1/(n D) sum_r w[t_r] sum_f m_rf rho(out_rf - target_rf)

The oracle zero-fills x0, runs ``O.training_forward(..., return_loss=False)`` once, applies torch's own reduction="none" losses and the
mask, and takes every gradient by autograd."""
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as O
from loss_helpers import L1_MARGIN, Fp64Oracle

# the shape groups of tests/test_gpu_loss.py (dims, hidden, rows): the smallest that reach each code path
REAL = (62, 5054, 26, 4)        # D = 5142, D % 4 == 2: the guarded epilogue and a ragged feature tile
FULL = (50, 1900, 50, 3)        # D = 2000: the transposer path; 2111 rows: squad forward, ragged last row block
DEEP = (16, 480, 16, 3)
H3 = [256, 512, 256]
H4 = [256, 256, 512, 256]
SHAPES = {
    "real16": dict(dims=REAL, hidden=H3, n=16, draw="injected"),
    "full2111": dict(dims=FULL, hidden=H3, n=2111, draw="philox"),
    "deep300": dict(dims=DEEP, hidden=H4, n=300, draw="philox"),
}
PROLOGUE_SHAPES = {"real16": (REAL, 16), "d2000x37": (FULL, 37)}      # case 1 of test_gpu_mask.py
FULL_ROW = 1                    # the row mask_pattern keeps fully observed


def mask_pattern(n, dims, seed=0):
    """bool [n, D], True = MISSING.  About 30 % of the rows lack the whole expression block (mutation-only patients), about 10 % of
    the elements are scattered, row 0 is entirely missing, row FULL_ROW is fully observed, and the last row's last D % 32 + 4 columns
    are missing (the ragged feature tile / guarded tail, in the ragged last row block)."""
    mut, expr, pw, _ = dims
    D = mut + expr + pw
    assert n >= 3
    g = torch.Generator().manual_seed(1000 + seed)
    miss = torch.rand(n, D, generator=g) < 0.10
    no_expr = torch.rand(n, generator=g) < 0.30
    miss[no_expr, mut:mut + expr] = True
    miss[0] = True
    miss[FULL_ROW] = False
    miss[n - 1, D - (D % 32 + 4):] = True
    return miss


def with_nan(x, miss):
    return torch.where(miss, torch.full_like(x, float("nan")), x)


def zero_fill(x):
    return torch.where(torch.isnan(x), torch.zeros_like(x), x)


def mix(x, cond, idx_a, idx_b, lam):
    """MixupAugmentation.mix / k_q_sample_src in fp32: lam * v[a] + (1 - lam) * v[b], NaN propagating -- a mixed element is observed
    iff both parents are."""
    return lam * x[idx_a] + (1 - lam) * x[idx_b], lam * cond[idx_a] + (1 - lam) * cond[idx_b]


def target_of(bufs, x0f, t, noise, prediction_type):
    """The training target on the zero-filled input, in the dtype of x0f."""
    a = bufs["sqrt_alphas_cumprod"][t].view(-1, 1).to(x0f.dtype)
    b = bufs["sqrt_one_minus_alphas_cumprod"][t].view(-1, 1).to(x0f.dtype)
    return {"epsilon": noise, "v_prediction": a * noise - b * x0f, "sample": x0f}[prediction_type]


class MaskedOracle:
    """fp64 loss and gradients of the masked objective for x0 with NaN = not observed."""

    def __init__(self, sd, x0, cond, t, noise, hidden, masks=None, p=0.0):
        self.observed = ~torch.isnan(x0)
        self.inner = Fp64Oracle(sd, zero_fill(x0), cond, t, noise, hidden, masks, p)

    @property
    def pred(self):
        return self.inner.pred

    def masked_loss(self, pred, kind, delta=1.0, weights=None, prediction_type="epsilon"):
        o = self.inner
        fn = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=delta)}[kind]
        per = fn(pred, target_of(o.bufs, o.x0, o.t, o.noise, prediction_type), reduction="none") * self.observed.double()
        if weights is not None:
            per = per * torch.as_tensor(weights).double()[o.t].view(-1, 1)
        return per.sum() / per.numel()

    def loss_and_grads(self, kind, delta=1.0, weights=None, prediction_type="epsilon"):
        return self.inner.grads_of(lambda pd: self.masked_loss(pd, kind, delta, weights, prediction_type))


class MixupMaskedOracle(MaskedOracle):
    """The same after a NaN-propagating fp32 mixup of rows idx_a with rows idx_b."""

    def __init__(self, sd, x, cond, idx_a, idx_b, lam, t, noise, hidden, masks=None, p=0.0):
        self.x_mix, self.cond_mix = mix(x, cond, idx_a, idx_b, lam)
        super().__init__(sd, self.x_mix, self.cond_mix, t, noise, hidden, masks, p)


def condition_l1_x0(pred_fn, x0, margin=L1_MARGIN, rounds=4):
    """loss_helpers.condition_l1_noise for the ``sample`` target: there d = out - x~0, so it is x0 that moves off L1's kink.  While an
    OBSERVED |d| < margin in float64, that element of x0 moves by 16 * margin away from the prediction; unobserved elements stay NaN
    (their zero-fill is what the prediction sees).  ``pred_fn(zero-filled fp32 x0) -> float64 prediction``.  Returns (fp32 x0 with
    its NaN, observed elements inside the margin round by round -- last entry 0 on success)."""
    x0 = x0.clone().float()
    observed = ~torch.isnan(x0)
    counts = []
    for _ in range(rounds + 1):
        xf = zero_fill(x0)
        d = pred_fn(xf) - xf.double()
        inside = (d.abs() < margin) & observed
        counts.append(int(inside.sum()))
        if counts[-1] == 0 or len(counts) > rounds:
            break
        away = torch.where(d >= 0, -1.0, 1.0).double() * (16.0 * margin)
        x0 = torch.where(inside, (xf.double() + away).float(), x0)
    return x0, counts


def q_sample_fp32(x0, t, noise, prediction_type, bufs=None):
    """The host fp32 restatement of the masked prologue: (x_t, target) with two rounded products and one add on the zero-filled input;
    the target carries NaN exactly where x0 does."""
    bufs = O.schedule_buffers("cosine", 1000) if bufs is None else bufs
    x0f = zero_fill(x0.float())
    a = bufs["sqrt_alphas_cumprod"].float()[t].view(-1, 1)
    b = bufs["sqrt_one_minus_alphas_cumprod"].float()[t].view(-1, 1)
    x_t = a * x0f + b * noise.float()
    return x_t, with_nan(target_of(bufs, x0f, t, noise.float(), prediction_type), torch.isnan(x0))
