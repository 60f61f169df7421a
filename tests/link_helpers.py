"""Shared pieces of the logistic-link tests (test_link_cpu.py, test_gpu_link.py, test_gpu_link_tiles.py): fp64 restatements of the link loss and of the link inside
the reverse chain, on top of loss_helpers.Fp64Oracle, pred_helpers.loss_fn / chain64 and mask_helpers.

    o = out, y = target (x0: the type is "sample"; inside [0, 1] after a mixup), M = mutation_dim
    f <  M:  rho = max(o, 0) - o y + log1p(exp(-|o|))         (F.binary_cross_entropy_with_logits, reduction="none")
    f >= M:  rho(o - y) of the configured loss_type           (pred_helpers.loss_fn's torch functions)
    loss = 1/(n D) sum_r w[t_r] sum_f m_rf rho_rf             m = observed (all ones without NaN)

Sampling: x0^ = sigma(out) on the columns f < M, out elsewhere, which for a "sample" model is an ``out_fn`` of chain64."""
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import objective as OB
from helpers import FULL_H
from loss_helpers import L1_MARGIN, P_DROP, Fp64Oracle, inputs, philox_masks, predict_fp64
from mask_helpers import H3, mask_pattern, with_nan, zero_fill
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


TILE_EDGES = (31, 32, 63, 64, 127, 128)      # the last / first column of a 32-column block, of a 64-column wave, of a 128-column tile


def boundary_columns(M, D, extra=()):
    """The columns the link boundary can go wrong at: [M - 8, M + 8), the block / wave / tile edges and ``extra``, inside [0, D)."""
    cols = set(range(M - 8, M + 8)) | set(TILE_EDGES) | {int(c) for c in extra}
    return sorted(c for c in cols if 0 <= c < D)


def check_boundary(grads, ref_grads, cols, rtol, atol=1e-9, show=None):
    """output_proj's bias gradient at ``cols`` and its weight-gradient rows at ``cols`` against the reference, element by element, each
    against the largest reference magnitude ON THOSE COLUMNS (loss_helpers.check takes the whole tensor's, which at 2 000 rows lets one
    mis-linked column through).  Returns (worst error / tolerance, failures) as loss_helpers.check does."""
    worst, bad = 0.0, []
    idx = torch.as_tensor(list(cols), dtype=torch.long)
    for key in ("unet.output_proj.bias", "unet.output_proj.weight"):
        got, ref = grads[key].detach().double()[idx], ref_grads[key].detach().double()[idx]
        tol = atol + rtol * ref.abs().max().item()
        d = (got - ref).abs()
        err = d.max().item() if bool(torch.isfinite(got).all()) else float("inf")
        at = int(idx[int(d.reshape(len(idx), -1).max(dim=1).values.argmax())])
        worst = max(worst, err / tol)
        if show:
            print(f"  [{show}] {key} at {len(idx)} boundary columns: max|d|={err:.3e} (column {at}) tol={tol:.3e} ratio={err / tol:.3f}")
        if not err <= tol:
            bad.append(f"{key} at the boundary columns: max|d|={err:.3e} (column {at}) > tol={tol:.3e}")
    return worst, bad


def fp32_link_grads(sd, x0, cond, t, noise, hidden, M, masks=None, p=0.0, kind="l2", delta=1.0, weights=None):
    """LinkOracle.loss_and_grads restated in torch fp32 -- forward, loss and autograd all in float32: what any fp32 implementation's
    rounding looks like next to the float64 oracle.  x0 with NaN = not observed.  Returns (loss, {name: gradient})."""
    observed = ~torch.isnan(x0)
    y = zero_fill(x0).float()
    bufs = {k: v.float() for k, v in O.schedule_buffers("cosine", 1000).items()}
    leaves = {k: v.detach().float().clone().requires_grad_(True) for k, v in sd.items()}
    pred = O.training_forward(leaves, bufs, y, cond.float(), t, noise.float(), len(hidden), 128,
                              None if masks is None else [m.float() for m in masks], p if masks is not None else 0.0, return_loss=False)
    cont = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=delta)}[kind]
    is_link = (torch.arange(y.shape[1]) < M).view(1, -1)
    per = torch.where(is_link, F.binary_cross_entropy_with_logits(pred, y, reduction="none"), cont(pred, y, reduction="none")) * observed.float()
    if weights is not None:
        per = per * torch.as_tensor(weights).float()[t].view(-1, 1)
    loss = per.sum() / per.numel()
    g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return loss.item(), {k: (torch.zeros_like(v) if gk is None else gk) for (k, v), gk in zip(leaves.items(), g)}


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


# ---- the shape groups of tests/test_gpu_link_tiles.py: the link boundary past the first wave tile ---------------------------------------
# D = 5142 (D % 4 = 2): the guarded epilogue; D = 2000: the transposer path; 2111 rows of it: 16 x 17 = 272 >= 256 tiles, the 128 x 128 tile
TILE_GROUPS = {
    "guard16": dict(D=5142, tail=(26, 4), n=16, draw="injected", Ms=(32, 64, 98, 130, 200)),
    "xpose37": dict(D=2000, tail=(50, 3), n=37, draw="philox", Ms=(32, 64, 98, 130, 200, 1950)),
    "big2111": dict(D=2000, tail=(50, 3), n=2111, draw="philox", Ms=(98, 200)),
}
# objective: (loss_type of the continuous columns, huber_delta, weighting, missing_values: mask)
TILE_OBJECTIVES = {"l2": ("l2", 1.0, None, False), "huber0.3-minsnr-masked": ("huber", 0.3, "min_snr", True), "l2-masked": ("l2", 1.0, None, True)}
SAT_COLS, SAT_BIAS = (0, 31, 64, 97), (100.0, -100.0, 40.0, -40.0)        # saturated logits: output_proj's bias on four link columns
_tile_cache = {}


def loss_weights(weighting):
    """The per-timestep weight table of a weighting: None, "min_snr" (gamma = 5, the sample form) or "custom"."""
    if weighting == "min_snr":
        return OB.min_snr_weights(O.schedule_buffers("cosine", 1000)["alphas_cumprod"], 5.0, "sample")
    if weighting == "custom":
        return torch.rand(1000, generator=torch.Generator().manual_seed(4)) * 2 + 0.05
    return None


def tile_dims(group, M):
    """(mutation, expression, pathway, condition) dims of a group with M link columns; D stays the group's."""
    g = TILE_GROUPS[group]
    if M == 1950:
        assert g["D"] == 2000
        return (1950, 24, 26, g["tail"][1])
    pw, cd = g["tail"]
    return (M, g["D"] - pw - M, pw, cd)


def tile_masks(group, injected):
    g = TILE_GROUPS[group]
    return injected if g["draw"] == "injected" else philox_masks(H3, g["n"])


def tile_shape(group, M, masked=False, sat=False):
    """(sd, x0 -- with NaN when masked --, cond, t, noise, injected masks, oracle) of a group at n_link = M: built once, left unchanged.
    sat: output_proj's bias at SAT_COLS is SAT_BIAS."""
    key = (group, M, masked, sat)
    if key not in _tile_cache:
        g = TILE_GROUPS[group]
        dims, n = tile_dims(group, M), g["n"]
        assert sum(dims[:3]) == g["D"]
        sd, x, cond, t, noise, injected = inputs(dims, H3, n)
        if sat:
            sd = dict(sd)
            bias = sd["unet.output_proj.bias"].clone()
            bias[list(SAT_COLS)] = torch.tensor(SAT_BIAS)
            sd["unet.output_proj.bias"] = bias
            for c in SAT_COLS:
                assert c < M and 0 < float(x[:, c].sum()) < n          # the targets 0 and 1 are both there
        masks = tile_masks(group, injected)
        if masked:
            x = with_nan(x, mask_pattern(n, dims))
        x, counts = condition_l1_x0_cont(lambda xf: predict_fp64(sd, xf, cond, t, noise, H3, masks, P_DROP), x, M)
        assert counts[-1] == 0, f"{key}: {counts[-1]} residuals are still within {L1_MARGIN} of the kink"
        xf = zero_fill(x)
        assert bool(((xf[:, :M] == 0) | (xf[:, :M] == 1)).all())
        _tile_cache[key] = (sd, x, cond, t, noise, injected, LinkOracle(sd, x, cond, t, noise, H3, M, masks, P_DROP))
    return _tile_cache[key]


def tile_reference(group, M, obj, sat=False, link=None):
    """fp64 (loss, gradients) of the objective; link: another number of link columns on the same forward graph (a control)."""
    key = ("ref", group, M, obj, sat, link)
    if key not in _tile_cache:
        kind, delta, weighting, masked = TILE_OBJECTIVES[obj]
        orc = tile_shape(group, M, masked, sat)[6]
        if link is None:
            _tile_cache[key] = orc.loss_and_grads(kind, delta, loss_weights(weighting))
        else:
            _tile_cache[key] = orc.inner.grads_of(link_loss_fn(orc.inner, link, kind, delta, loss_weights(weighting), orc.observed))
    return _tile_cache[key]
