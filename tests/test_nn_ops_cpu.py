"""CPU: what test_gpu_nn_ops.py stands on (nn_ops_helpers.py).  The float64 references equal torch's own fp32 modules to fp32
accuracy; every seed and shape the GPU file feeds the BatchNorm -> ReLU -> Dropout block keeps its live pre-activations MARGIN away
from the ReLU gate (and forces at most FORCED_CAP of the mask to do so); and the fp32 torch-autograd error of the reparameterisation
gradient on the extreme-range inputs, which the GPU test is measured against, is what nn_ops_helpers records."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nn_ops_helpers as H
from helpers import assert_close

FP32 = 2e-6          # a handful of fp32 roundings relative to max|ref|; the K = 2004 dot products get sqrt(K) of them


@pytest.mark.parametrize("shape", [s for s, _ in H.LINEAR_SHAPES], ids=[i for _, i in H.LINEAR_SHAPES])
def test_linear_reference_vs_torch_fp32(shape):
    n, K1, K2, N = shape
    x1, x2, w, b, gy = H.linear_inputs(n, K1, K2, N)
    lin = torch.nn.Linear(K1 + K2, N)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    xin = x1.clone().requires_grad_(True)
    y = lin(xin if x2 is None else torch.cat([xin, x2], dim=1))
    y.backward(gy)
    ref = H.linear_ref(x1, x2, w, b, gy)
    assert x1.mean().abs() > 0.1 and abs(float(((x1 - x1.mean()) ** 3).mean())) > 0 and w.shape == (N, K1 + K2)
    for got, want, what in zip((y, xin.grad, lin.weight.grad, lin.bias.grad), ref, ("y", "dx1", "dw", "db")):
        assert_close(got, want, FP32 * max(1.0, (K1 + K2) ** 0.5 / 8), what=what)


def _torch_block(c, training, use_bn, p):
    """torch's own fp32 modules on the case's inputs: (y, dz, dgamma, dbeta, bn)."""
    n, C = c["z"].shape
    z = c["z"].clone().requires_grad_(True)
    bn = None
    pre = z
    if use_bn:
        bn = torch.nn.BatchNorm1d(C, eps=H.BN_EPS, momentum=H.MOMENTUM)
        with torch.no_grad():
            bn.weight.copy_(c["gamma"])
            bn.bias.copy_(c["beta"])
            bn.running_mean.copy_(c["rm"])
            bn.running_var.copy_(c["rv"])
        bn.train(bool(training))
        pre = bn(z)
    y = torch.nn.ReLU()(pre)
    if c["mask"] is not None and training:
        y = y * c["mask"] / (1.0 - p)
    y.backward(c["gy"])
    return y.detach(), z.grad, (bn.weight.grad if bn else None), (bn.bias.grad if bn else None), bn


def _compare_block(c, training, use_bn, p):
    ref = H.block_ref(c["z"], c["gy"], c["gamma"] if use_bn else None, c["beta"], c["rm"], c["rv"], training, c["mask"], p)
    y, dz, dgamma, dbeta, bn = _torch_block(c, training, use_bn, p)
    assert_close(y, ref["y"], 1e-5, what="y")
    assert_close(dz, ref["dz"], 5e-5, atol=3e-6, what="dz")
    if use_bn:
        assert_close(dgamma, ref["dgamma"], 5e-5, atol=3e-6, what="dgamma")
        assert_close(dbeta, ref["dbeta"], 5e-5, atol=3e-6, what="dbeta")
        assert_close(bn.running_mean, ref["running_mean"], 1e-6, what="running_mean")
        assert_close(bn.running_var, ref["running_var"], 1e-6, what="running_var")
        z64 = c["z"].double()
        if training:      # the saved statistics are what they are named
            assert torch.equal(ref["save_mean"], z64.mean(0))
            assert torch.allclose(ref["save_invstd"], 1 / torch.sqrt(((z64 - z64.mean(0)) ** 2).mean(0) + H.BN_EPS), rtol=1e-12, atol=0)


# (4099, 257) is left to the margin test below: torch's fp32 BatchNorm on a million elements adds nothing about the reference
@pytest.mark.parametrize("n,C", [s for s in H.BLOCK_MASKED_SHAPES if s[0] * s[1] < 1 << 18])
def test_block_reference_vs_torch_fp32_masked(n, C):
    _compare_block(H.masked_case(n, C), True, True, H.P_DROP)


@pytest.mark.parametrize("n,C", H.BLOCK_P0_SHAPES)
def test_block_reference_vs_torch_fp32_p0(n, C):
    _compare_block(H.p0_case(n, C), True, True, 0.0)


@pytest.mark.parametrize("n,C", [s for s in H.BLOCK_EVAL_SHAPES if s[0] * s[1] < 1 << 18])
def test_block_reference_vs_torch_fp32_eval(n, C):
    _compare_block(H.eval_case(n, C), False, True, H.P_DROP)


@pytest.mark.parametrize("n,C", H.BLOCK_NOBN_SHAPES)
def test_block_reference_vs_torch_fp32_nobn(n, C):
    _compare_block(H.nobn_case(n, C), True, False, H.P_DROP)


def test_block_reference_unbiased_factor():
    """n = 2: running_var takes var_biased * n / (n - 1) = 2 var_biased."""
    c = H.masked_case(2, 3)
    ref = H.block_ref(c["z"], c["gy"], c["gamma"], c["beta"], c["rm"], c["rv"], True, c["mask"], H.P_DROP)
    vb = c["z"].double().var(0, unbiased=False)
    assert torch.allclose(ref["running_var"], (1 - H.MOMENTUM) * c["rv"].double() + H.MOMENTUM * 2.0 * vb, rtol=1e-13, atol=0)
    _compare_block(c, True, True, H.P_DROP)


# ---- the conditions of the ReLU gate (nn_ops_helpers' docstring) -----------------------------------------------------------------
@pytest.mark.parametrize("n,C,stress", [(n, C, False) for n, C in H.BLOCK_MASKED_SHAPES] + [(257, 65, True), (2, 3, False)])
def test_masked_cases_force_few_drops_and_leave_no_live_element_at_the_gate(n, C, stress):
    c = H.masked_case(n, C, stress=stress)
    pre = H.pre64(c["z"], c["gamma"], c["beta"], c["rm"], c["rv"], True)
    live = c["mask"] > 0
    share = c["forced"] / (n * C)
    print(f"masked ({n}, {C}) stress={stress}: forced {c['forced']} of {n * C} ({100 * share:.4f} %), live min|pre| = "
          f"{float(pre.abs()[live].min()) if live.any() else float('nan'):.3e}")
    assert share <= H.FORCED_CAP                       # below a thousand elements this allows none
    assert not live.any() or float(pre.abs()[live].min()) >= H.MARGIN
    assert set(np.unique(c["mask"].numpy())) <= {0.0, 1.0}
    if n * C >= 300:
        assert 0.7 < float(c["mask"].mean()) < 0.9          # still a p = 0.2 mask
    if stress:
        z = c["z"].double()
        assert float(z[:, 3].var(unbiased=False)) == 0.0 and abs(float(z[:, 7].mean()) - 30) < 0.01 and 0.02 < float(z[:, 7].std()) < 0.04


@pytest.mark.parametrize("n,C", H.BLOCK_P0_SHAPES)
def test_checked_seeds_keep_the_margin(n, C):
    c = H.p0_case(n, C)
    pre = H.pre64(c["z"], c["gamma"], c["beta"], c["rm"], c["rv"], True)
    print(f"p = 0 ({n}, {C}) seed {H.CHECKED_SEED[(n, C)]}: min|pre| = {float(pre.abs().min()):.3e}")
    assert float(pre.abs().min()) >= H.MARGIN


@pytest.mark.parametrize("n,C", H.BLOCK_EVAL_SHAPES)
def test_eval_cases_keep_the_margin_after_the_nudge(n, C):
    c = H.eval_case(n, C)
    pre = H.pre64(c["z"], c["gamma"], c["beta"], c["rm"], c["rv"], False)
    print(f"eval ({n}, {C}): nudged {c['nudged']} of {n * C}, min|pre| = {float(pre.abs().min()):.3e}")
    assert float(pre.abs().min()) >= H.MARGIN
    assert c["nudged"] <= max(1, H.FORCED_CAP * n * C)


def test_seeded_dropout_reference_is_a_p_mask():
    for (n, C), tag, p in zip(H.SEEDED_DROPOUT_SHAPES, (0x11, 0x2A, 0x11), (0.2, 0.5, 0.2)):
        k = H.keep_mask(99, n, C, tag, p)
        assert k.shape == (n, C) and set(np.unique(k.numpy())) <= {0.0, 1.0}
        if n * C > 10000:
            assert abs(float(k.mean()) - (1 - p)) < 5 * (p * (1 - p) / (n * C)) ** 0.5
    assert not torch.equal(H.keep_mask(99, 257, 65, 0x11, 0.2), H.keep_mask(99, 257, 65, 0x2A, 0.2))


# ---- reparameterisation and the losses ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Lz", [s for s in H.REPARAM_SHAPES if s[0] * s[1] < 1 << 18])
def test_reparam_reference_vs_torch_fp32(n, Lz):
    mu, lv, eps, gz = H.reparam_inputs(n, Lz)
    z64, dmu64, dlv64 = H.reparam_ref(mu, lv, eps, gz)
    z32, dmu32, dlv32 = H.reparam_ref(mu, lv, eps, gz, torch.float32)
    assert_close(z32, z64, FP32, what="z")
    assert torch.equal(dmu64, gz.double()) and torch.equal(dmu32, gz)
    assert_close(dlv32, dlv64, FP32, what="d_logvar")


def test_reparam_extreme_range_fp32_autograd_error():
    """What the device d_logvar is measured against on a tight posterior far from the origin: torch's own fp32 autograd holds every
    element to a few roundings (it multiplies gz eps exp(0.5 lv) 0.5, it never subtracts), while 0.5 gz (z - mu) on the same fp32
    numbers loses every digit of some elements."""
    mu, lv, eps, gz = H.reparam_extreme_inputs()
    err = H.reparam_extreme_fp32_err()
    ref = H.reparam_ref(mu, lv, eps, gz)[2]
    z32 = H.reparam_ref(mu, lv, eps, None, torch.float32)
    cancelling = H.worst_rel(0.5 * gz * (z32 - mu), ref)
    print(f"extreme-range d_logvar, worst element: torch fp32 autograd {err:.3e}; 0.5 gz (z - mu) in fp32 {cancelling:.3e}; "
          f"recorded {H.REPARAM_EXTREME_FP32_ERR:.1e}")
    assert 2.0 ** -26 < err <= 2.0 ** -22           # three products and an exp, each within an ulp
    assert 0.5 * H.REPARAM_EXTREME_FP32_ERR <= err <= 2.0 * H.REPARAM_EXTREME_FP32_ERR    # exp differs by an ulp between hosts
    assert cancelling > 1e-2                         # the formula the kernel used to run: this is what the GPU test must catch
    assert float(mu.abs().max()) > 60 and -16 < float(lv.min()) and float(lv.max()) < -8


@pytest.mark.parametrize("n,D,Lz", H.VAE_LOSS_SHAPES)
def test_vae_loss_reference_vs_torch_fp32(n, D, Lz):
    xr, x, mu, lv = H.vae_loss_inputs(n, D, Lz)
    parts, d_recon, d_mu, d_lv = H.vae_loss_ref(xr, x, mu, lv)
    xr32, mu32, lv32 = (t.clone().requires_grad_(True) for t in (xr, mu, lv))
    recon = F.mse_loss(xr32, x, reduction="sum") / n                   # models/cvae.py:178-181
    kl = -0.5 * torch.sum(1 + lv32 - mu32.pow(2) - lv32.exp()) / n
    (recon + kl).backward()
    assert_close(recon.item(), parts[1], 1e-5, what="recon")
    assert_close(kl.item(), parts[2], 1e-5, atol=H.kl_atol(mu, lv), what="kl")
    assert_close((recon + kl).item(), parts[0], 1e-5, atol=H.kl_atol(mu, lv), what="total")
    assert parts[0] == parts[1] + parts[2]
    for got, want, what in ((xr32.grad, d_recon, "d_recon"), (mu32.grad, d_mu, "d_mu"), (lv32.grad, d_lv, "d_lv")):
        assert_close(got, want, 5e-5, atol=3e-6, what=what)


@pytest.mark.parametrize("count", H.MSE_COUNTS)
def test_mse_reference_vs_torch_fp32(count):
    a, b = H.mse_inputs(count)
    loss, da = H.mse_ref(a, b)
    a32 = a.clone().requires_grad_(True)
    l32 = F.mse_loss(a32, b)
    l32.backward()
    assert_close(l32.item(), loss, 1e-5, what="mse")
    assert_close(a32.grad, da, 5e-5, atol=3e-6, what="da")


def test_latent_noise_is_standard_normal():
    e = H.latent_noise(4242, 257, 130)
    assert e.shape == (257, 130) and abs(e.mean()) < 5 / e.size ** 0.5 and abs(e.var() - 1) < 5 * (2 / e.size) ** 0.5
