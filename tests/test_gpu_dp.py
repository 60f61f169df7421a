"""GPU: differentially private training -- per-row gradient norms, the clipped batch gradient, the refusals, the
noise of the DP optimizer step and the Trainer's ``training.dp`` -- against the float64 oracle of dp_helpers.py at the training
tolerances of loss_helpers.py (loss 1e-5, each gradient tensor 5e-5 of its max; a row's norm inherits the gradients' 5e-5).

Shapes: n = 70 rows (tails against 32- and 64-row tiles), D = 93 (D % 32 = 29, rows of d_out / x_t off the 16-byte grid), hidden
(256, 512, 256), train mode with injected keep-masks; cond_dim 4 and 8 are the two paths of the first embedding Linear's weight gradient
(the small kernel / the immediate GEMM).  The squad case is the smallest n and D whose backward runs as squads."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import objective as OB
from osteosarcoma_diffusionmodel_amd import privacy as PV
from osteosarcoma_diffusionmodel_amd.train import Trainer, _loss_fwd_bwd
from helpers import RawHandle, assert_close, config, philox_normals
from loss_helpers import GRAD_RTOL, LOSS_RTOL, P_DROP, SEED, check, inputs
from dp_helpers import DpOracle, choose_C

pytestmark = pytest.mark.gpu

SQ_BWD, DP_CLIP = 1 << 1, 1 << 13      # include/osdiff.h: OSD_TP_*
H3 = [256, 512, 256]
N = 70
DIMS4, DIMS8 = (6, 83, 4, 4), (6, 83, 4, 8)
D = 93
_cache = {}


def _min_snr():
    return OB.min_snr_weights(O.schedule_buffers("cosine", 1000)["alphas_cumprod"], 5.0)


def _model(dims, sd, hidden=H3, **diffusion):
    mut, expr, pw, cd = dims
    conf = config(hidden, p=P_DROP)
    conf["model"]["diffusion"].update(diffusion)
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    return m.cuda().train()


def _path(m):
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(m._engine().handle, b"last_train_path", C.byref(v)))
    return int(v.value)


def _call(m, x, cond, t, noise, masks, clip, **kw):
    """One training call with gradients: (loss, {name: gradient}, last_train_path, s_r or None)."""
    m.dp_max_grad_norm = clip
    grads = [torch.empty_like(p) for p in m.parameters()]
    loss = _loss_fwd_bwd(m, None if x is None else x.cuda(), None if cond is None else cond.cuda(), L.ptr_array(grads), t=t.cuda(),
                         noise=noise.cuda(), dropout_masks=[k.cuda() for k in masks], seed=SEED, **kw)
    torch.cuda.synchronize()
    norms = m.last_row_norms(t.shape[0]).cpu().double() if clip else None
    names = [k for k, _ in m.named_parameters()]
    return loss.item(), {k: g.cpu() for k, g in zip(names, grads)}, _path(m), norms


def _oracle(key, dims, n, **kw):
    """The shape's inputs and its oracle (built once, left unchanged): (sd, x, cond, t, noise, masks, oracle)."""
    if key not in _cache:
        sd, x, cond, t, noise, masks = inputs(dims, H3, n, seed=kw.pop("seed", 17))
        x, cond = kw.pop("x", x), kw.pop("cond", cond)
        _cache[key] = (sd, x, cond, t, noise, masks, DpOracle(sd, x, cond, t, noise, H3, masks, P_DROP, **kw))
    return _cache[key]


# ---- 1. row norms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [DIMS4, DIMS8], ids=["cond4", "cond8"])
def test_row_norms_vs_oracle(dims):
    sd, x, cond, t, noise, masks, orc = _oracle(("base", dims), dims, N)
    ref = orc.norms()
    m = _model(dims, sd)
    _, _, path, got = _call(m, x, cond, t, noise, masks, choose_C(ref))
    rel = ((got - ref).abs() / ref).max().item()
    print(f"[cond_dim {dims[3]}] s_r in [{ref.min():.4g}, {ref.max():.4g}], worst relative error {rel:.3e} (bar {GRAD_RTOL})")
    assert path & DP_CLIP
    assert rel <= GRAD_RTOL
    again = _call(m, x, cond, t, noise, masks, choose_C(ref))[3]
    assert np.array_equal(got.numpy(), again.numpy()), "two calls on the same inputs gave different norms"


# ---- 2. clipped gradients ------------------------------------------------------------------------------------------------------------
def _keep_vec():
    return (torch.rand(N, generator=torch.Generator().manual_seed(9)) >= 0.5).float()


C0 = np.array([0.3, -0.2, 0.5, 0.1], dtype=np.float32)      # the null condition of the condition-dropout case
CLIP_CASES = {
    # name: (model attributes, diffusion config keys, oracle keywords)
    "per-layer": (dict(train_squad=0), {}, {}),
    "bf16x3": (dict(precision="bf16x3"), {}, {}),
    "huber-minsnr": ({}, dict(loss_type="huber", huber_delta=0.7, loss_weighting="min_snr"), dict(kind="huber", delta=0.7, weights="min_snr")),
    "v_prediction": ({}, dict(prediction_type="v_prediction"), dict(prediction="v_prediction")),
    "cond-drop": ({}, {}, {}),
    "source": ({}, {}, {}),
}


@pytest.mark.parametrize("case", list(CLIP_CASES))
def test_clipped_gradients_vs_oracle(case):
    attrs, diffusion, okw = CLIP_CASES[case]
    okw = dict(okw)
    if okw.get("weights") == "min_snr":
        okw["weights"] = _min_snr()
    sd, x, cond, t, noise, masks = inputs(DIMS4, H3, N)
    call_kw, xin, cin = {}, x, cond
    if case == "cond-drop":
        keep = _keep_vec()
        okw["cond"] = torch.where(keep.view(-1, 1) > 0, cond, torch.from_numpy(C0).view(1, -1))
        call_kw["cond_drop"] = (C0, 0.5, keep.cuda())
    if case == "source":
        gen = torch.Generator().manual_seed(21)
        data, conds = torch.randn(100, D, generator=gen), torch.randn(100, 4, generator=gen)
        idx = torch.randperm(100, generator=gen)[:N]
        okw["x"], okw["cond"] = data[idx], conds[idx]
        call_kw["source"] = (data.cuda(), conds.cuda(), idx.cuda(), None, 1.0)
        xin = cin = None
    key = ("clip", case) if okw else ("base", DIMS4)
    orc = _oracle(key, DIMS4, N, **okw)[6]
    clip = choose_C(orc.norms())           # asserts a quarter clipped, a quarter not, no row within 1e-3 of C (on the CPU)
    ref = orc.clipped(clip)
    m = _model(DIMS4, sd, **diffusion)
    for k, v in attrs.items():
        setattr(m, k, v)
    loss, grads, path, norms = _call(m, xin, cin, t, noise, masks, clip, **call_kw)
    worst, bad = check(loss, grads, orc.loss(), ref, D)
    print(f"[{case}] C {clip:.5g}, loss {loss:.8g} (fp64 {orc.loss():.8g}), worst error / tolerance {worst:.3f}, path {path:#x}")
    assert not bad, "\n".join(bad)
    assert path & DP_CLIP, f"last_train_path {path:#x}"
    assert ((norms - orc.norms()).abs() / orc.norms()).max().item() <= GRAD_RTOL
    # the unclipped gradient is NOT within the tolerances: the case would notice a clip that did nothing
    _, plain = orc.orc.grads_of(lambda pd: orc._rows(pd).mean())
    assert check(loss, grads, orc.loss(), plain, D)[1], "the clipped gradient passes as the unclipped one"


# ---- 3. squads -------------------------------------------------------------------------------------------------------------------
def test_clipped_gradients_with_the_squad_backward():
    """The smallest batch whose dgrad chain runs as one launch of squads (2 048 rows): the leaves wait for the clip factors there too.
    D = 253, not the 93 of the other cases: a squad plan needs at least eight 32-column tiles of the state (train_squad_ok: D >= 225), and
    253 is the smallest such D with the same D % 32 = 29.  2 048 norms lie ~3e-4 (relative) apart near their median, so a C with no row
    within 1e-3 of it needs an unusually wide gap: the input recipe's seed 31 is the first from its default 17 on whose middle half has
    one (choose_C checks it, on the CPU)."""
    n, dims, d = 2048, (6, 243, 4, 4), 253
    sd, x, cond, t, noise, masks, orc = _oracle(("squad",), dims, n, seed=31)
    clip = choose_C(orc.norms())
    m = _model(dims, sd)
    loss, grads, path, norms = _call(m, x, cond, t, noise, masks, clip)
    worst, bad = check(loss, grads, orc.loss(), orc.clipped(clip), d)
    print(f"[squads] C {clip:.5g}, worst error / tolerance {worst:.3f}, path {path:#x}")
    assert path & SQ_BWD and path & DP_CLIP, f"last_train_path {path:#x}"
    assert not bad, "\n".join(bad)
    assert ((norms - orc.norms()).abs() / orc.norms()).max().item() <= GRAD_RTOL


# ---- 4. limits ---------------------------------------------------------------------------------------------------------------------
def test_huge_bound_and_cleared_bound():
    sd, x, cond, t, noise, masks = inputs(DIMS4, H3, N)
    fresh = _model(DIMS4, sd)
    l0, g0, p0, _ = _call(fresh, x, cond, t, noise, masks, None)
    m = _model(DIMS4, sd)
    l1, g1, p1, s1 = _call(m, x, cond, t, noise, masks, 1e30)
    assert p1 & DP_CLIP and not p0 & DP_CLIP
    worst, bad = check(l1, g1, l0, g0, D)
    assert not bad, "\n".join(bad)
    assert torch.isfinite(s1).all() and (s1 > 0).all()
    # cleared: today's launches.  The weight gradients of the grouped launch -- a fixed-order slab sum, no float atomic anywhere on their
    # way -- must come back bit for bit: every 2-D weight but time_proj's (a product of the atomically scattered time-table gradient) and
    # the first embedding Linear's (the small kernel adds its blocks' partials atomically).  The vectors (biases and GroupNorm affines:
    # atomic column sums) and those two are held to the 1e-6 a repeated sum of a few hundred terms moves by.
    l2, g2, p2, _ = _call(m, x, cond, t, noise, masks, None)
    assert p2 == p0, f"last_train_path {p2:#x} after clearing, {p0:#x} on a handle that never set the bound"
    strict = [k for k, v in g0.items() if v.dim() == 2 and k not in ("unet.time_proj.weight", "condition_embed.mlp.0.weight")]
    assert len(strict) == 14 and "unet.input_proj.weight" in strict and "unet.output_proj.weight" in strict
    for k in g0:
        if k in strict:
            assert torch.equal(g2[k], g0[k]), f"{k} differs after osd_set_dp_clip(h, 0)"
        else:
            assert_close(g2[k], g0[k], 1e-6, what=k)
    assert abs(l2 - l0) <= 1e-6 * abs(l0)


# ---- 5. sensitivity ----------------------------------------------------------------------------------------------------------------
def test_sensitivity_of_the_clipped_sum():
    """Replace one record; t, noise and masks of all rows stay.  |n G - n G'| <= 2 C + GRAD_RTOL (|n G| + |n G'|): what DP rests on."""
    sd, x, cond, t, noise, masks, orc = _oracle(("base", DIMS4), DIMS4, N)
    clip = choose_C(orc.norms())
    gen = torch.Generator().manual_seed(77)
    x2, c2 = x.clone(), cond.clone()
    r = int(orc.norms().argmax())                      # the row with the largest gradient: the replacement matters most
    x2[r], c2[r] = 3.0 * torch.randn(D, generator=gen), torch.randn(4, generator=gen)
    m = _model(DIMS4, sd)
    ga = _call(m, x, cond, t, noise, masks, clip)[1]
    gb = _call(m, x2, c2, t, noise, masks, clip)[1]
    flat = lambda g: torch.cat([v.double().reshape(-1) for v in g.values()]) * N
    a, b = flat(ga), flat(gb)
    diff, bound = (a - b).norm().item(), 2 * clip + GRAD_RTOL * (a.norm().item() + b.norm().item())
    print(f"|nG - nG'| = {diff:.5g}, 2C = {2 * clip:.5g}, |nG| = {a.norm().item():.5g}")
    assert 0 < diff <= bound


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["events", "loss_scale", "constraints", "mixup-source", "hidden-64"])
def test_refusals_touch_no_gradient(case):
    hidden = [64, 128, 64] if case == "hidden-64" else H3
    sd, x, cond, t, noise, masks = inputs(DIMS4, hidden, N)
    m = _model(DIMS4, sd, hidden)
    m.dp_max_grad_norm = 1.0
    kw = dict(t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in masks], seed=SEED)
    xin, cin = x.cuda(), cond.cuda()
    if case == "events":
        kw["events"] = [torch.cuda.Event() for _ in range(len(hidden) * 2 - 1 + 2)]
        for e in kw["events"]:
            e.record()
    if case == "loss_scale":
        kw["loss_scale"] = 0.5
    if case == "constraints":
        m.set_constraints(pathways=[[10, 11, 12], [20, 21]], pathway_weight=0.5)
    if case == "mixup-source":
        idx = torch.arange(N).cuda()
        kw["source"] = (xin, cin, idx, idx.flip(0).contiguous(), 0.7)
        xin = cin = None
    grads = [torch.full_like(p, 7.0) for p in m.parameters()]
    with pytest.raises(ValueError, match="per-row gradient clipping"):
        _loss_fwd_bwd(m, xin, cin, L.ptr_array(grads), **kw)
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in grads), "a refused call wrote into a gradient buffer"
    # the same call without gradients (validation) is none of the mode's business
    if case not in ("events", "mixup-source"):
        kw.pop("events", None)
        assert np.isfinite(_loss_fwd_bwd(m, xin, cin, None, **kw).item())


def test_denoiser_backward_refuses_while_a_bound_is_set():
    """The autograd path for a caller's own loss cannot know whether its rows are per-patient terms: no unclipped gradients from it."""
    sd, x, cond, t, noise, masks = inputs(DIMS4, H3, N)
    m = _model(DIMS4, sd)
    m.dp_max_grad_norm = 1.0
    h = m._engine().handle
    grads = [torch.full_like(p, 7.0) for p in m.parameters()]
    xt, t32, c, dout = x.cuda(), t.to(torch.int32).cuda(), cond.cuda(), noise.cuda()
    rc = L.lib().osd_denoiser_backward(h, L.ptr(xt), L.ptr(t32), L.ptr(c), N, L.ptr(dout), None, SEED, 0, 0, L.ptr_array(grads), None, None, 0)
    assert rc == L.OSD_EUNSUPPORTED and "osd_set_dp_clip" in L.last_error()
    torch.cuda.synchronize()
    assert all(bool((g == 7.0).all()) for g in grads)


def test_bad_bounds_and_state():
    h = RawHandle()
    try:
        lib = L.lib()
        for bad in (-1.0, float("nan"), float("inf")):
            assert lib.osd_set_dp_clip(h.h, bad) == L.OSD_EINVAL
        assert lib.osd_set_dp_clip(h.h, 0.0) == L.OSD_OK and lib.osd_set_dp_clip(h.h, 2.5) == L.OSD_OK
        out = torch.zeros(4, device="cuda")
        assert lib.osd_dp_row_norms(h.h, L.ptr(out), 4) == L.OSD_ESTATE
    finally:
        h.close()


# ---- 7. noise ---------------------------------------------------------------------------------------------------------------------
def _host_noise(seed, step, numel):
    rows = (numel + L.DP_NOISE_COLS - 1) // L.DP_NOISE_COLS
    return philox_normals(seed, rows, L.DP_NOISE_COLS, step, L.DP_NOISE_TAG).reshape(-1)[:numel]


def lerp32(e, p, decay):
    """One EMA update as the kernels round it (tests/test_gpu_ema.py); e, p float32 arrays."""
    w32 = np.float32(1.0 - decay)
    return e + w32 * (p - e)


@pytest.mark.parametrize("variant, off", [("plain", 0), ("ema-nn", 0), ("ema-handle", 0), ("ema-nn", 1)],
                         ids=["plain", "ema-nn", "ema-handle", "ema-unaligned"])
def test_dp_adamw_step(variant, off):
    """Noise = the host's Philox restatement for the (rows, 4096) reading of the flat buffer, at the 2e-5 absolute bar on a normal of
    test_randn_matches_host_philox; AdamW on the noised gradient at the tolerances of test_fused_clip_adamw_vs_torch; the average as
    test_kernel_ema_bit_for_bit holds it: bit for bit the host's three-rounding lerp of the parameter the step has just produced, from a
    start unrelated to the parameters, while parameters, gradient and moments equal the step without the average bit for bit.
    n is odd (the scalar tail); off = 1 starts every buffer one float behind a 16-byte boundary (the scalar fallback)."""
    gen = torch.Generator().manual_seed(5)
    n, std, seed, lr, wd = 100003, 0.05, (3 << 33) + 12345, 1e-3, 1e-2
    ema = variant != "plain"

    def buf(src=None):
        t = torch.zeros(n + 8, device="cuda")[off:off + n]
        assert t.data_ptr() % 16 == 4 * off
        if src is not None:
            t.copy_(src)
        return t

    p0, g0, e0 = torch.randn(n, generator=gen), 1e-3 * torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    p, g, mm, vv, e = buf(p0), buf(g0), buf(), buf(), buf(e0)
    pt, gt, mt, vt = buf(p0), buf(g0), buf(), buf()                      # the twin without the average
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=lr, weight_decay=wd)
    stream, dev = C.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.current_device()
    lib = L.lib()
    h = RawHandle()
    try:
        e_host = e0.numpy().copy()
        for step, decay in enumerate([0.9, 2.0 / 11.0, 0.999, 1.0, 0.0], start=1):
            g.copy_(g0)
            gt.copy_(g0)
            hyper = (n, lr, 0.9, 0.999, 1e-8, wd, std, seed, step)
            L.check(lib.osd_nn_dp_adamw_step(stream, dev, L.ptr(pt), L.ptr(gt), L.ptr(mt), L.ptr(vt), *hyper))
            if variant == "plain":
                L.check(lib.osd_dp_adamw_step(h.h, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), *hyper))
            elif variant == "ema-nn":
                L.check(lib.osd_nn_dp_adamw_ema_step(stream, dev, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), L.ptr(e), *hyper, decay))
            else:
                L.check(lib.osd_dp_adamw_ema_step(h.h, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), L.ptr(e), *hyper, decay))
            torch.cuda.synchronize()
            for name, a_, b_ in (("param", p, pt), ("grad", g, gt), ("exp_avg", mm, mt), ("exp_avg_sq", vv, vt)):
                assert np.array_equal(a_.cpu().numpy(), b_.cpu().numpy()), f"{name} differs from the step without the average at step {step}"
            z = (g.cpu().double() - g0.double()).numpy() / std
            assert np.abs(z - _host_noise(seed, step, n)).max() <= 2e-5, f"step {step}"
            ref.grad = g.cpu().clone()
            opt.step()
            assert_close(p.cpu(), ref.detach(), 1e-6, what=f"param step {step}")
            if ema:
                before = e_host
                e_host = lerp32(e_host, p.cpu().numpy(), decay)
                got = e.cpu().numpy()
                assert np.array_equal(got, e_host), f"ema at step {step} (decay {decay}): {np.count_nonzero(got != e_host)} of {n} differ"
                if decay == 1.0:
                    assert np.array_equal(got, before)
            else:
                assert np.array_equal(e.cpu().numpy(), e0.numpy())          # never touched
        assert_close(mm.cpu(), opt.state[ref]["exp_avg"], 1e-6)
        assert_close(vv.cpu(), opt.state[ref]["exp_avg_sq"], 5e-6)
        if ema:
            assert np.isfinite(e_host).all() and not np.array_equal(e_host, e0.numpy())
            assert lib.osd_dp_adamw_ema_step(h.h, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), None, n, lr, 0.9, 0.999, 1e-8, wd, std, seed, 6, 0.9) == L.OSD_EINVAL
            assert lib.osd_dp_adamw_ema_step(h.h, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), L.ptr(e), n, lr, 0.9, 0.999, 1e-8, wd, std, seed, 6, 1.5) == L.OSD_EINVAL
        # noise_std 0: nothing added, the gradient left as it was; a bad argument is refused
        g.copy_(g0)
        L.check(lib.osd_dp_adamw_step(h.h, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), n, lr, 0.9, 0.999, 1e-8, wd, 0.0, seed, 6))
        assert torch.equal(g.cpu(), g0)
        assert lib.osd_dp_adamw_step(h.h, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), n, lr, 0.9, 0.999, 1e-8, wd, -1.0, seed, 7) == L.OSD_EINVAL
    finally:
        h.close()


def test_dp_noise_statistics_and_keys():
    n, std, seed = 1 << 20, 0.25, 991
    stream, dev = C.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.current_device()

    def draw(seed, step):
        p, g, mm, vv = (torch.zeros(n, device="cuda") for _ in range(4))
        L.check(L.lib().osd_nn_dp_adamw_step(stream, dev, L.ptr(p), L.ptr(g), L.ptr(mm), L.ptr(vv), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, std, seed, step))
        torch.cuda.synchronize()
        return g.cpu().double().numpy()

    a, b, c, d = draw(seed, 7), draw(seed, 7), draw(seed, 8), draw(seed + 1, 7)
    assert np.array_equal(a, b), "the same (seed, step) gave other noise"
    assert np.abs(a - c).max() > std and np.abs(a - d).max() > std and abs(np.corrcoef(a, c)[0, 1]) < 5 / np.sqrt(n)
    mean, var = a.mean(), a.var()
    print(f"mean {mean:.3e} (se {std / np.sqrt(n):.3e}), var {var:.6f} (noise_std^2 {std * std:.6f})")
    assert abs(mean) <= 5 * std / np.sqrt(n)
    assert abs(var - std * std) <= 5 * std * std * np.sqrt(2.0 / n)
    assert np.abs(a / std - _host_noise(seed, 7, n)).max() <= 2e-5


# ---- 8. Trainer -------------------------------------------------------------------------------------------------------------------
class _Rows(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {"data": torch.zeros(D), "conditions": torch.zeros(4), "survival": torch.zeros(())}


def _trainer(tmp_path, sd, dp, **extra):
    conf = config(H3, p=P_DROP)
    conf["training"] = {"learning_rate": 1e-3, "weight_decay": 1e-2, "patience": 5, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.0},
                        "save_dir": str(tmp_path), "num_epochs": 3, "save_frequency": 10, "val_split": 0.2, "random_seed": 1, "batch_size": N,
                        "dp": dp, **extra}
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=6, expression_dim=83, pathway_dim=4, condition_dim=4)
    m.load_state_dict(sd, strict=False)
    loader = torch.utils.data.DataLoader(_Rows(4 * N), batch_size=N, drop_last=True)
    return Trainer(m, loader, [], conf, device="cuda")


def test_trainer_dp_step(tmp_path):
    """One train_step = the oracle's clipped gradient + the host's noise, then AdamW.  The noised gradient the step writes back is held to
    GRAD_RTOL max|G_k| + 2e-5 noise_std per tensor (the two bars it inherits); the update is then checked as torch.optim.AdamW fed THAT
    gradient, at test_fused_clip_adamw_vs_torch's tolerances -- Adam's first step is lr * sign(g), so feeding it the oracle's gradient would
    turn every element whose noised gradient lies within rounding of zero into a full 2 lr difference."""
    sd, x, cond, t, noise, masks, orc = _oracle(("base", DIMS4), DIMS4, N)
    clip, sigma, seed = choose_C(orc.norms()), 1.1, 4242
    tr = _trainer(tmp_path / "a", sd, {"max_grad_norm": clip, "noise_multiplier": sigma, "delta": 1e-5, "seed": seed})
    assert tr.optimizer.max_norm == 0.0 and tr.model.dp_max_grad_norm == clip
    before = tr.flat.flat.cpu().clone()
    loss = tr.train_step(x.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in masks], seed=SEED)
    torch.cuda.synchronize()
    assert abs(loss.item() - orc.loss()) <= LOSS_RTOL * abs(orc.loss())
    norms = tr.last_row_norms().cpu().double()
    assert ((norms - orc.norms()).abs() / orc.norms()).max().item() <= GRAD_RTOL
    std = sigma * clip / N
    z = _host_noise(seed, 1, tr.flat.flat.numel())
    ref = orc.clipped(clip)
    names = [k for k, _ in tr.model.named_parameters()]
    for k, gv, o, cnt in zip(names, tr.flat.grad_views, tr.flat.offsets[:-1], tr.flat.numels):
        want = ref[k].reshape(-1).numpy() + std * z[int(o):int(o) + cnt]
        err = np.abs(gv.cpu().double().reshape(-1).numpy() - want).max()
        assert err <= GRAD_RTOL * ref[k].abs().max().item() + 2e-5 * std + 1e-9, f"{k}: {err:.3e}"
    p = torch.nn.Parameter(before.clone())
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=1e-2)
    p.grad = tr.flat.grad.cpu().clone()
    opt.step()
    assert_close(tr.flat.flat.cpu(), p.detach(), 1e-6, what="parameters after the DP step")
    # the account
    spent = tr.privacy_spent()
    assert spent == {"epsilon": PV.epsilon(N / (4 * N), sigma, 1, 1e-5), "delta": 1e-5, "steps": 1, "sample_rate": 0.25, "noise_multiplier": sigma}
    tr.train_step(x.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in masks], seed=SEED)
    assert tr.privacy_spent()["epsilon"] == PV.epsilon(0.25, sigma, 2, 1e-5) > spent["epsilon"]
    # checkpoint round trip: the step count, hence the account, survives
    tr.save_checkpoint(0, 1.0)
    ck = torch.load(tmp_path / "a" / "checkpoint_epoch_0.pt", map_location="cpu", weights_only=True)
    assert ck["dp_state"]["steps"] == 2 and ck["dp_state"]["noise_multiplier"] == sigma
    other = _trainer(tmp_path / "b", sd, {"max_grad_norm": clip, "noise_multiplier": sigma, "delta": 1e-5, "seed": seed})
    assert other.privacy_spent()["steps"] == 0
    other.load_checkpoint(tmp_path / "a" / "checkpoint_epoch_0.pt")
    assert other.privacy_spent() == tr.privacy_spent() and other.optimizer._step == 2
    # a resume under another sigma would price the saved steps wrongly: refused, nothing loaded
    wrong = _trainer(tmp_path / "e", sd, {"max_grad_norm": clip, "noise_multiplier": 2.0, "delta": 1e-5, "seed": seed})
    w_before = wrong.flat.flat.clone()
    with pytest.raises(ValueError, match="noise_multiplier"):
        wrong.load_checkpoint(tmp_path / "a" / "checkpoint_epoch_0.pt")
    assert torch.equal(wrong.flat.flat, w_before) and wrong.privacy_spent()["steps"] == 0
    # target_epsilon: sigma for the planned 3 epochs x 4 batches
    planned = _trainer(tmp_path / "c", sd, {"max_grad_norm": clip, "target_epsilon": 4.0})
    s = planned.dp["noise_multiplier"]
    assert PV.epsilon(0.25, s, 12, 1e-5) <= 4.0 <= PV.epsilon(0.25, s * 0.98, 12, 1e-5)
    # absent: the keys and the batch clip of today
    plain = _trainer(tmp_path / "d", sd, None)
    assert plain.dp is None and plain.optimizer.max_norm == 1.0 and plain.model.dp_max_grad_norm is None
    plain.save_checkpoint(0, 1.0)
    assert set(torch.load(tmp_path / "d" / "checkpoint_epoch_0.pt", map_location="cpu", weights_only=True)) == \
        {"epoch", "model_state_dict", "optimizer_state_dict", "val_loss", "config"}
    with pytest.raises(RuntimeError):
        plain.privacy_spent()


def test_trainer_dp_with_ema(tmp_path):
    """training.dp together with training.ema_decay: the average rides in the DP optimizer step -- bit for bit the host's lerp of the
    parameters that step produced (that the step itself equals the one without an average is test_dp_adamw_step's twin)."""
    sd, x, cond, t, noise, masks, orc = _oracle(("base", DIMS4), DIMS4, N)
    dp = {"max_grad_norm": choose_C(orc.norms()), "noise_multiplier": 1.1, "delta": 1e-5, "seed": 4242}
    tr = _trainer(tmp_path / "a", sd, dict(dp), ema_decay=0.99)
    assert tr.ema is not None and tr.optimizer.ema is tr.ema and tr.optimizer.dp is not None
    e_host = tr.ema.shadow.cpu().numpy().copy()
    assert np.array_equal(e_host, tr.flat.flat.cpu().numpy())
    for k in (1, 2, 3):
        tr.train_step(x.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda(), dropout_masks=[m.cuda() for m in masks], seed=SEED + k)
        torch.cuda.synchronize()
        e_host = lerp32(e_host, tr.flat.flat.cpu().numpy(), tr.ema.decay_at(k))
        assert np.array_equal(tr.ema.shadow.cpu().numpy(), e_host), f"shadow after step {k}"
    assert tr.ema.num_updates == 3 == tr.privacy_spent()["steps"]
    assert tr.optimizer.max_norm == 0.0 and float(tr.optimizer.grad_norm.item()) == 0.0          # the DP step ran, not the clipping one
    assert not np.array_equal(e_host, tr.flat.flat.cpu().numpy())


def test_replay_refuses_a_stale_workspace():
    """osd_dp_replay (the bench aid) relaunches on workspace pointers: only right after a clipped call whose conditions sat in the
    workspace, never after another call has carved it again."""
    sd, x, cond, t, noise, masks = inputs(DIMS4, H3, N)
    m = _model(DIMS4, sd)
    lib, h = L.lib(), m._engine().handle
    _call(m, x, cond, t, noise, masks, 5.0)                                   # conditions = the caller's tensor
    assert lib.osd_dp_replay(h, 0, 0.0) == L.OSD_ESTATE
    idx = torch.arange(N).cuda()
    _call(m, None, None, t, noise, masks, 1e30, source=(x.cuda(), cond.cuda(), idx, None, 1.0))          # no row scaled: a replay reads what the call read
    before = m.last_row_norms(N).clone()
    assert lib.osd_dp_replay(h, 0, 0.0) == L.OSD_OK
    torch.cuda.synchronize()
    assert torch.equal(m.last_row_norms(N), before)                           # the same launch on the same buffers: the same bits
    _call(m, x[:40], cond[:40], t[:40], noise[:40], [k[:40] for k in masks], None)      # another call carves the workspace
    assert lib.osd_dp_replay(h, 0, 0.0) == L.OSD_ESTATE and lib.osd_dp_replay(h, 1, 0.0) == L.OSD_ESTATE
