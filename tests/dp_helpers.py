"""Shared pieces of the differentially-private-training tests (test_dp_cpu.py, test_gpu_dp.py): the float64 oracle of per-row gradient
norms and of the clipped batch gradient, the choice of the bound C, and a quadrature of the accountant's moment.

Definitions: a call on n rows has loss L = (1/n) sum_r l_r, l_r = (1/D) w[t_r] sum_f rho(d_rf); g_r = grad l_r over
all parameter tensors as one vector, s_r = |g_r|_2, c_r = min(1, C / (s_r + 1e-6)), G = (1/n) sum_r c_r g_r.

The DEFINITION is ``brute``: one ``autograd.grad`` of l_r per row through ``O.training_forward``'s graph (loss_helpers.Fp64Oracle).  The
vectorised form, for the larger cases: s_r from the row-norm identity on a restated forward that keeps every Linear's (input, output)
and every GroupNorm's (zhat, output), and G as the gradient of (1/n) sum_r c_r l_r with the c_r as constants, through the oracle's own
graph.  test_dp_cpu.py shows the two equal to 1e-10."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import diffusion_oracle as O
from loss_helpers import Fp64Oracle

CLIP_EPS = 1e-6
C_MARGIN = 1e-3           # no row's norm within this relative distance of C: a row on the edge would flip between clipped and not


def target_of(orc, prediction):
    """What the prediction is compared with: eps, or v = sqrt(abar) eps - sqrt(1 - abar) x0."""
    if prediction == "epsilon":
        return orc.noise
    assert prediction == "v_prediction"
    sa = orc.bufs["sqrt_alphas_cumprod"][orc.t].view(-1, 1)
    s1 = orc.bufs["sqrt_one_minus_alphas_cumprod"][orc.t].view(-1, 1)
    return sa * orc.noise - s1 * orc.x0


def row_losses(pred, target, t, kind="l2", delta=1.0, weights=None):
    """l_r [n] = (1/D) w[t_r] sum_f rho(pred_rf - target_rf), rho from torch's own loss functions."""
    fn = {"l2": F.mse_loss, "l1": F.l1_loss, "huber": lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=delta)}[kind]
    per = fn(pred, target, reduction="none")
    if weights is not None:
        per = per * torch.as_tensor(weights).double()[t].view(-1, 1)
    return per.sum(1) / per.shape[1]


def clip_factors(norms, C):
    return torch.clamp(C / (norms + CLIP_EPS), max=1.0)


class DpOracle:
    """Float64 per-row norms and the clipped batch gradient of one training call."""

    def __init__(self, sd, x0, cond, t, noise, hidden, masks=None, p=0.0, *, kind="l2", delta=1.0, weights=None, prediction="epsilon"):
        self.orc = Fp64Oracle(sd, x0, cond, t, noise, hidden, masks, p)
        self.sd, self.hidden, self.loss_args, self.prediction = sd, hidden, (kind, delta, weights), prediction
        self.n = x0.shape[0]
        self._norms = None

    def _rows(self, pred):
        return row_losses(pred, target_of(self.orc, self.prediction), self.orc.t, *self.loss_args)

    def loss(self):
        return self._rows(self.orc.pred.detach()).mean().item()

    # ---- the definition -----------------------------------------------------------------------------------------------------
    def brute(self, C):
        """(s_r [n], {name: G}) from one autograd.grad per row."""
        leaves = list(self.orc.leaves.values())
        rows = self._rows(self.orc.pred)
        norms = torch.zeros(self.n, dtype=torch.float64)
        total = [torch.zeros_like(v) for v in leaves]
        for r in range(self.n):
            g = torch.autograd.grad(rows[r], leaves, retain_graph=True, allow_unused=True)
            g = [torch.zeros_like(v) if gk is None else gk for v, gk in zip(leaves, g)]
            norms[r] = math.sqrt(sum(float((gk * gk).sum()) for gk in g))
            c = min(1.0, C / (norms[r].item() + CLIP_EPS))
            for acc, gk in zip(total, g):
                acc += c * gk
        return norms, {k: acc / self.n for k, acc in zip(self.orc.leaves, total)}

    # ---- the vectorised form --------------------------------------------------------------------------------------------------
    def norms(self):
        """s_r [n] from the row-norm identity: a Linear z = x W^T + b contributes (|x_r|^2 + 1) |dL/dz_r|^2, a GroupNorm's affine
        sum_c (gy_rc zhat_rc)^2 + gy_rc^2 with gy = dL/d(its output); L = sum_r l_r so that row r of every dL/d. is row r's own."""
        if self._norms is None:
            o = self.orc
            sd = {k: v.detach().clone().requires_grad_(True) for k, v in o.leaves.items()}      # leaves of a graph of its own
            lins, gns = [], []

            def linear(x, name):
                z = F.linear(x, sd[f"{name}.weight"], sd[f"{name}.bias"])
                lins.append((x.detach(), z))
                return z

            def half(x, prefix, li, gi):
                z = linear(x, f"{prefix}.{li}")
                y = F.group_norm(z, O.GN_GROUPS, sd[f"{prefix}.{gi}.weight"], sd[f"{prefix}.{gi}.bias"], O.GN_EPS)
                gns.append((F.group_norm(z.detach(), O.GN_GROUPS, None, None, O.GN_EPS), y))
                return F.silu(y)

            T = o.bufs["betas"].shape[0]
            x_t = O.q_sample(o.bufs, o.x0, o.t, o.noise)
            u = linear(o.cond, "condition_embed.mlp.0")
            c_emb = linear(F.silu(u), "condition_embed.mlp.2")
            h = linear(x_t, "unet.input_proj") + linear(O.time_embedding(o.t.double() / T, 128), "unet.time_proj") + linear(c_emb, "unet.cond_proj")
            names, n_enc, skips = O.block_names(len(self.hidden)), len(self.hidden) - 1, []
            for bi, name in enumerate(names):
                if bi > n_enc:
                    h = torch.cat([h, skips.pop()], dim=-1)
                a = half(h, name, 0, 1)
                if o.masks is not None:
                    a = a * (o.masks[bi] / (1.0 - o.p))
                h = half(a, name, 4, 5)
                if bi < n_enc:
                    skips.append(h)
            pred = linear(h, "unet.output_proj")
            assert torch.allclose(pred, o.pred.detach(), rtol=1e-12, atol=1e-12), "the restated forward differs from O.training_forward"
            outs = [z for _, z in lins] + [y for _, y in gns]
            gs = torch.autograd.grad(self._rows(pred).sum(), outs)
            sq = torch.zeros(self.n, dtype=torch.float64)
            for (x, _), d in zip(lins, gs[:len(lins)]):
                sq += ((x * x).sum(1) + 1.0) * (d * d).sum(1)
            for (zh, _), gy in zip(gns, gs[len(lins):]):
                sq += ((gy * zh) ** 2).sum(1) + (gy * gy).sum(1)
            self._norms = sq.sqrt()
        return self._norms

    def clipped(self, C, norms=None):
        """{name: G}: the gradient of (1/n) sum_r c_r l_r, c_r constants, through the oracle's own graph."""
        c = clip_factors(self.norms() if norms is None else norms, C)
        _, g = self.orc.grads_of(lambda pd: (c * self._rows(pd)).sum() / self.n)
        return g


def choose_C(norms):
    """The median norm; if a row lies within C_MARGIN (relative) of it, the middle of the nearest gap between two adjacent norms that
    keeps every row outside the margin and at least a quarter of the rows on either side.  Raises AssertionError if there is none."""
    s = np.sort(np.asarray(norms, dtype=np.float64))
    n = len(s)
    C = float(np.median(s))
    if np.any(np.abs(s - C) <= C_MARGIN * C):
        lo, hi = -(-n // 4), n - -(-n // 4)          # C between s[k] and s[k + 1] clips n - k - 1 rows: lo <= k + 1 <= hi
        order = sorted(range(max(lo - 1, 0), min(hi, n - 1)), key=lambda k: abs(k - (n // 2 - 1)))
        for k in order:
            mid = 0.5 * (s[k] + s[k + 1])
            if s[k + 1] - mid > C_MARGIN * mid and mid - s[k] > C_MARGIN * mid:
                C = float(mid)
                break
        else:
            raise AssertionError(f"no gap between adjacent norms of the middle half is wider than {2 * C_MARGIN} relative")
    assert not np.any(np.abs(s - C) <= C_MARGIN * C)
    clipped = int((s > C).sum())
    assert clipped >= n / 4 and n - clipped >= n / 4, f"{clipped} of {n} rows clipped at C = {C}"
    return C


def moment_quadrature(q, sigma, alpha, points=100_001):
    """log E_{z ~ mu0}[(mu / mu0)^alpha], mu0 = N(0, sigma^2), mu = (1 - q) mu0 + q N(1, sigma^2), by the trapezoid rule (spectrally
    accurate for this integrand) on a grid wide enough for its mass, which sits near z = alpha for large alpha.  For small q the moment is
    1 + O(q^2): the quadrature is of (mu / mu0)^alpha - 1, and log1p of it, so that the 1 does not eat the digits."""
    lo, hi = -40.0 * sigma, 40.0 * sigma + alpha
    z = np.linspace(lo, hi, points)
    l0 = -z * z / (2 * sigma * sigma)
    l1 = -(z - 1.0) ** 2 / (2 * sigma * sigma)
    lr = np.logaddexp(math.log1p(-q) + 0.0 * z, math.log(q) + l1 - l0)
    a = alpha * lr
    small = a < 1.0          # expm1 where it keeps digits, the plain difference where it would overflow
    f = np.where(small, np.expm1(np.where(small, a, 0.0)) * np.exp(l0), np.exp(a + l0) - np.exp(l0)) / (sigma * math.sqrt(2 * math.pi))
    dz = (hi - lo) / (points - 1)
    return math.log1p(math.fsum(f[1:-1]) * dz + 0.5 * (f[0] + f[-1]) * dz)
