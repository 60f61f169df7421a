"""GPU: the logistic link on the mutation block -- cross-entropy on the logits inside the fused training step,
sigma on the unfolded x0 inside the sampling step -- against float64 restatements (link_helpers.py on loss_helpers.Fp64Oracle,
pred_helpers.chain64 and test_solver_cpu.dpmpp_chain).

Training: the shape groups of mask_helpers.SHAPES, the project's training tolerances (loss 1e-5 relative, each gradient tensor
max|d| <= 5e-5 * max|ref| + 1e-9 and the same on the tail columns / rows: loss_helpers.check).  The continuous columns of x0 are moved
off L1's kink (link_helpers.condition_l1_x0_cont); the link loss is smooth and its 0 / 1 targets stay.
Sampling: the case of tests/test_known_cpu.py (make_case, PLAN, N) at tol_of's tolerance, 5e-5 * max|ref| + 1e-5: sigma' <= 1/4, so
the link cannot amplify an error of the output."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table, ddim_timesteps, ddim_x0_table, dpmpp_2m_table, known_level_table
from osteosarcoma_diffusionmodel_amd.train import _loss_fwd_bwd
from helpers import FULL_H, assert_close, config
from link_helpers import LinkOracle, condition_l1_x0_cont, link_eps_fn, link_out, loss_weights
from loss_helpers import GRAD_RTOL, L1_MARGIN, LOSS_RTOL, P_DROP, SEED, Fp64Oracle, check, inputs, philox_masks, predict_fp64
from mask_helpers import DEEP, H4, SHAPES, mask_pattern, mix, with_nan, zero_fill
from pred_helpers import chain64, guided_out, model_sd64
from test_clip_cpu import mixed_bounds
from test_gpu_ddim import _model as ddim_model, _use
from test_gpu_known import C0_NONZERO
from test_known_cpu import ATOL, MD, N, PLAN, RTOL, T, make_case, make_known, tol_of
from test_solver_cpu import dpmpp_chain

pytestmark = pytest.mark.gpu

SQ_FWD, XPAD, MSE_BF16, LOSS_EPI, MASKED, LINK = 1 << 0, 1 << 6, 1 << 10, 1 << 11, 1 << 14, 1 << 15      # include/osdiff.h: OSD_TP_*
S = 10
_cache = {}


# ======== training ======================================================================================================================
_weights = loss_weights


def _shape(name, masked=False):
    """(sd, x0 -- with NaN when masked --, cond, t, noise, injected masks, oracle) of a shape group: built once, left unchanged."""
    key = (name, masked)
    if key not in _cache:
        s = SHAPES[name]
        M = s["dims"][0]
        sd, x, cond, t, noise, injected = inputs(s["dims"], s["hidden"], s["n"])
        masks = injected if s["draw"] == "injected" else philox_masks(s["hidden"], s["n"])
        if masked:
            x = with_nan(x, mask_pattern(s["n"], s["dims"]))
        x, counts = condition_l1_x0_cont(lambda xf: predict_fp64(sd, xf, cond, t, noise, s["hidden"], masks, P_DROP), x, M)
        print(f"[{name} masked={masked}] continuous residuals inside the L1 margin, round by round: {counts}")
        assert counts[-1] == 0, f"{name}: {counts[-1]} residuals are still within {L1_MARGIN} of L1's kink"
        xf = zero_fill(x)
        assert bool(((xf[:, :M] == 0) | (xf[:, :M] == 1)).all())          # the link targets stay 0 / 1
        orc = LinkOracle(sd, x, cond, t, noise, s["hidden"], M, masks, P_DROP)
        _cache[key] = (sd, x, cond, t, noise, injected, orc)
    return _cache[key]


def _model(name, sd, link="logistic", missing_values=None, precision=None, **diffusion):
    s = SHAPES[name]
    mut, expr, pw, cd = s["dims"]
    conf = config(s["hidden"], p=P_DROP)
    conf["model"]["diffusion"].update(prediction_type="sample", **diffusion)
    if link is not None:
        conf["model"]["diffusion"]["mutation_link"] = link
    if missing_values is not None:
        conf["training"] = {"missing_values": missing_values}
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    m.precision = precision
    return m


def _option(m, name):
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(m._engine().handle, name, C.byref(v)))
    return int(v.value)


def _run(name, m, masked=False, x=None, cond=None, source=None, with_grads=True):
    """(loss, {name: gradient} or None, last_train_path) of one training call of ``m`` with the shape group's t / noise / masks."""
    s = SHAPES[name]
    sd, x0, cond0, t, noise, injected, _ = _shape(name, masked)
    grads = [torch.empty_like(p) for p in m.parameters()] if with_grads else None
    kw = dict(t=t.cuda(), noise=noise.cuda(), seed=SEED)
    if s["draw"] == "injected":
        kw["dropout_masks"] = [k.cuda() for k in injected]
    if source is not None:
        loss = _loss_fwd_bwd(m, None, None, None if grads is None else L.ptr_array(grads), source=source, **kw)
    else:
        loss = _loss_fwd_bwd(m, (x0 if x is None else x).cuda(), (cond0 if cond is None else cond).cuda(),
                             None if grads is None else L.ptr_array(grads), **kw)
    torch.cuda.synchronize()
    names = [k for k, _ in m.named_parameters()]
    return loss.item(), None if grads is None else {k: g.cpu() for k, g in zip(names, grads)}, _option(m, b"last_train_path")


def _compare(name, tag, got, ref):
    worst, bad = check(got[0], got[1], ref[0], ref[1], sum(SHAPES[name]["dims"][:3]), show=tag)
    print(f"[{name} {tag}] loss {got[0]:.8g} (fp64 {ref[0]:.8g}); worst error / tolerance {worst:.3f}")
    return bad


# (shape group, loss_type of the continuous columns, huber_delta, weighting, missing_values: mask, path bits set, path bits clear)
CASES = {
    "real16-l2": ("real16", "l2", 1.0, None, False, 0, SQ_FWD | XPAD | MSE_BF16),
    "real16-l1-custom": ("real16", "l1", 1.0, "custom", False, 0, SQ_FWD | XPAD | MSE_BF16),
    "real16-huber0.3-minsnr-masked": ("real16", "huber", 0.3, "min_snr", True, MASKED, SQ_FWD | XPAD | MSE_BF16),
    "full2111-l2-custom": ("full2111", "l2", 1.0, "custom", False, SQ_FWD | XPAD, MSE_BF16),
    "full2111-l1-minsnr": ("full2111", "l1", 1.0, "min_snr", False, SQ_FWD | XPAD, MSE_BF16),
    "full2111-l2-masked": ("full2111", "l2", 1.0, None, True, SQ_FWD | XPAD | MASKED, MSE_BF16),
    "deep300-huber-minsnr": ("deep300", "huber", 1.0, "min_snr", False, 0, SQ_FWD | XPAD | MSE_BF16),
    "deep300-l1": ("deep300", "l1", 1.0, None, False, 0, SQ_FWD | XPAD | MSE_BF16),
}


def _reference(case):
    if ("ref", case) not in _cache:
        name, kind, delta, weighting, masked, _, _ = CASES[case]
        _cache[("ref", case)] = _shape(name, masked)[6].loss_and_grads(kind, delta, _weights(weighting))
    return _cache[("ref", case)]


def _case_model(case, precision=None):
    name, kind, delta, weighting, masked, _, _ = CASES[case]
    m = _model(name, _shape(name, masked)[0], missing_values="mask" if masked else None, precision=precision, loss_type=kind,
               huber_delta=delta, loss_weighting="min_snr" if weighting == "min_snr" else None)
    if weighting == "custom":
        m.set_loss_weights(_weights("custom"))
    return m


@pytest.mark.parametrize("case", list(CASES))
def test_link_loss_vs_fp64_autograd(case):
    name, kind, delta, weighting, masked, want_set, want_clear = CASES[case]
    ref = _reference(case)
    M = SHAPES[name]["dims"][0]
    m = _case_model(case)
    got = _run(name, m, masked)
    bad = _compare(name, case, got, ref)
    assert not bad, "\n".join(bad)
    path = got[2]
    assert path & LINK and path & LOSS_EPI, f"last_train_path {path:#x}: the link epilogue did not run"
    assert path & want_set == want_set and not path & want_clear, f"last_train_path {path:#x}, wanted {want_set:#x} set and {want_clear:#x} clear"
    assert _option(m, b"output_link") == M
    # a loss-only call (no gradient buffers) returns the same loss
    only = _run(name, m, masked, with_grads=False)
    assert_close(only[0], ref[0], LOSS_RTOL, what="loss-only call")
    assert abs(only[0] - got[0]) <= 1e-6 * abs(got[0])
    assert only[2] & LINK


def test_negative_controls_training():
    """The tolerance separates: the device's link loss against the oracle without a link, against the oracle whose link columns keep
    l2's folded 2 in the gradient, and (masked) against the oracle that counts ln 2 for every unobserved link element."""
    name = "real16"
    got = _run(name, _case_model("real16-l2"))
    orc = _shape(name)[6]
    M = orc.M
    assert _compare(name, "control: no link", got, orc.inner.loss_and_grads("l2")), "a missing link went unnoticed"
    is_link = (torch.arange(orc.pred.shape[1]) < M).view(1, -1)

    def doubled(pred):          # the same loss value, the link columns' gradient doubled
        import torch.nn.functional as F
        bce = F.binary_cross_entropy_with_logits(pred, orc.inner.x0, reduction="none")
        per = torch.where(is_link, 2 * bce - bce.detach(), (pred - orc.inner.x0) ** 2)
        return per.sum() / per.numel()
    ref2 = orc.inner.grads_of(doubled)
    assert abs(ref2[0] - _reference("real16-l2")[0]) <= 1e-12 * abs(ref2[0])
    assert _compare(name, "control: folded 2", got, ref2), "a doubled link gradient went unnoticed"
    case = "real16-huber0.3-minsnr-masked"
    got_m = _run(name, _case_model(case), True)
    orc_m = _shape(name, True)[6]
    leaked = LinkOracle.__new__(LinkOracle)
    leaked.M, leaked.inner = M, orc_m.inner
    leaked.observed = orc_m.observed | is_link           # unobserved link elements count rho(0 - 0) ... of the zero-filled target
    assert _compare(name, "control: leaked ln 2", got_m, leaked.loss_and_grads("huber", 0.3, _weights("min_snr"))), "a leak went unnoticed"


def test_mixup_batch_source_targets_inside_the_unit_interval():
    """osd_train_batch_source with idx_b set, lam = 0.3, at deep300: the link targets are 0, 0.3, 0.7 or 1."""
    name, lam = "deep300", 0.3
    sd, x, cond, t, noise, injected, _ = _shape(name)
    n, M = SHAPES[name]["n"], DEEP[0]
    g = torch.Generator().manual_seed(11)
    idx_a, perm = torch.randperm(n, generator=g), torch.randperm(n, generator=g)
    idx_b = idx_a[perm]
    x_mix, cond_mix = mix(x, cond, idx_a, idx_b, lam)
    inside = (x_mix[:, :M] > 0) & (x_mix[:, :M] < 1)
    assert float(inside.double().mean()) > 0.2, "no link target strictly inside (0, 1)"
    ref = LinkOracle(sd, x_mix, cond_mix, t, noise, H4, M, philox_masks(H4, n), P_DROP).loss_and_grads("l2")
    got = _run(name, _model(name, sd), source=(x.cuda(), cond.cuda(), idx_a.cuda(), idx_b.cuda(), lam))
    bad = _compare(name, "resident source + mixup", got, ref)
    assert not bad, "\n".join(bad)
    assert got[2] & LINK and got[2] & LOSS_EPI


def test_bf16x3_keeps_the_link_loss_on_the_fp32_launcher():
    case = "full2111-l2-custom"
    name = CASES[case][0]
    got = _run(name, _case_model(case, precision="bf16x3"))
    bad = _compare(name, "bf16x3", got, _reference(case))
    assert not bad, "\n".join(bad)
    assert got[2] & LINK and not got[2] & MSE_BF16, f"last_train_path {got[2]:#x}"


def _small_call(link):
    """tests/test_gpu_loss.py's reproducible shape with prediction_type sample: (loss, gradients, path, output_link)."""
    dims, hidden, n = (8, 24, 8, 3), [32, 64, 32], 16
    sd, x, cond, t, noise, injected = inputs(dims, hidden, n)
    mut, expr, pw, cd = dims
    conf = config(hidden, p=P_DROP)
    conf["model"]["diffusion"]["prediction_type"] = "sample"
    if link is not None:
        conf["model"]["diffusion"]["mutation_link"] = link
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    grads = [torch.empty_like(p) for p in m.parameters()]
    loss = _loss_fwd_bwd(m, x.cuda(), cond.cuda(), L.ptr_array(grads), t=t.cuda(), noise=noise.cuda(), seed=SEED,
                         dropout_masks=[k.cuda() for k in injected])
    torch.cuda.synchronize()
    return loss.cpu(), [g.cpu() for g in grads], _option(m, b"last_train_path"), _option(m, b"output_link"), m


def test_identity_is_the_model_without_the_key():
    base, again, named = _small_call(None), _small_call(None), _small_call("identity")
    assert torch.equal(base[0], again[0]) and all(torch.equal(p, q) for p, q in zip(base[1], again[1])), "the step is not reproducible here"
    assert torch.equal(base[0], named[0]) and all(torch.equal(p, q) for p, q in zip(base[1], named[1]))
    assert base[2] == named[2] and not base[2] & LINK and base[3] == named[3] == 0
    linked = _small_call("logistic")
    assert linked[2] & LINK and linked[3] == 8 and not torch.equal(linked[0], base[0])
    # a live model switched logistic -> identity has the bits of a fresh identity model, and the handle's link is off again
    m = linked[4]
    m.mutation_link = "identity"
    dims, hidden, n = (8, 24, 8, 3), [32, 64, 32], 16
    sd, x, cond, t, noise, injected = inputs(dims, hidden, n)
    grads = [torch.empty_like(p) for p in m.parameters()]
    loss = _loss_fwd_bwd(m, x.cuda(), cond.cuda(), L.ptr_array(grads), t=t.cuda(), noise=noise.cuda(), seed=SEED,
                         dropout_masks=[k.cuda() for k in injected])
    torch.cuda.synchronize()
    assert torch.equal(loss.cpu(), base[0]) and all(torch.equal(g.cpu(), q) for g, q in zip(grads, base[1]))
    assert _option(m, b"output_link") == 0 and _option(m, b"last_train_path") == base[2]
    # ... and logistic -> epsilon in one assignment pair: the link goes off before the type leaves sample
    m.mutation_link = "logistic"
    m._engine()
    m.mutation_link, m.prediction_type = "identity", "epsilon"
    m._engine()
    assert _option(m, b"output_link") == 0 and _option(m, b"prediction_type") == L.OSD_PRED_EPSILON


def test_training_refusals_on_the_device_path():
    name = "deep300"
    sd, x, cond, t, noise, injected, _ = _shape(name)
    mut = DEEP[0]
    m = _model(name, sd)
    eng = m._engine()
    lib = L.lib()
    sentinel = [torch.full_like(p, 7.0) for p in m.parameters()]
    xd, cd_, td, nd = x.cuda(), cond.cuda(), t.cuda().int(), noise.cuda()
    loss = torch.zeros(1, device="cuda")

    def raw_call():
        rc = lib.osd_train_loss_fwd_bwd(eng.handle, L.ptr(xd), L.ptr(cd_), x.shape[0], L.ptr(td), L.ptr(nd), None, SEED, 0, 0, L.ptr(loss),
                                        L.ptr_array(sentinel), 1.0, None, 0)
        torch.cuda.synchronize()
        return rc

    # the library's own refusals (the Python layer refuses the same earlier): constraint losses, per-row clipping, the row mode
    m.set_constraints([[mut + 1, mut + 7, mut + 100]], list(range(4)), list(range(mut, mut + 4)), pathway_weight=0.5, mutexpr_weight=0.5)
    eng.set_constraints(m._constraints)
    assert raw_call() == L.OSD_EUNSUPPORTED and "osd_set_output_link" in L.last_error()
    m.set_constraints()
    eng.set_constraints(None)
    L.check(lib.osd_set_dp_clip(eng.handle, 1.0))
    assert raw_call() == L.OSD_EUNSUPPORTED and "osd_set_output_link" in L.last_error()
    L.check(lib.osd_set_dp_clip(eng.handle, 0.0))
    se = torch.empty(x.shape[0], device="cuda")
    assert lib.osd_row_sq_error(eng.handle, L.ptr(xd), L.ptr(cd_), x.shape[0], L.ptr(td), L.ptr(nd), 0, 0, L.ptr(se)) == L.OSD_EUNSUPPORTED
    assert "osd_set_output_link" in L.last_error()
    assert all(bool((g == 7.0).all()) for g in sentinel)
    # osd_set_output_link's own checks; either setting can come second
    D = m.data_dim
    assert lib.osd_set_output_link(eng.handle, -1) == L.OSD_EINVAL and lib.osd_set_output_link(eng.handle, D + 1) == L.OSD_EINVAL
    assert lib.osd_set_output_link(eng.handle, D) == L.OSD_OK and _option(m, b"output_link") == D
    assert lib.osd_set_output_link(eng.handle, mut) == L.OSD_OK
    L.check(lib.osd_set_prediction(eng.handle, L.OSD_PRED_V))          # the type set second
    assert raw_call() == L.OSD_EINVAL and "osd_set_prediction" in L.last_error()
    assert lib.osd_set_output_link(eng.handle, 0) == L.OSD_OK
    assert lib.osd_set_output_link(eng.handle, mut) == L.OSD_EINVAL and "OSD_PRED_SAMPLE" in L.last_error()      # the link set second
    L.check(lib.osd_set_prediction(eng.handle, L.OSD_PRED_SAMPLE))
    assert lib.osd_set_output_link(eng.handle, mut) == L.OSD_OK
    assert all(bool((g == 7.0).all()) for g in sentinel)
    # the handle is still usable: the oracle's loss and gradients
    got = _run(name, m)
    bad = _compare(name, "after the refusals", got, _shape(name)[6].loss_and_grads("l2"))
    assert not bad, "\n".join(bad)


# ======== sampling ======================================================================================================================
def chain_link(m, cond, *, lo=None, hi=None, x_T=None, zs=None, seed=0, row_offset=0, taus=None, eta=0.0, null=None, w=1.0, known=None,
               expect=L.OSD_OK):
    """osd_sample_chain_clipped through ctypes on the model's handle with the tables of a sample model: (x_out, mutation mask).
    taus = None is the DDPM chain; lo = hi = None are infinite bounds."""
    eng = m._engine()
    n, D = cond.shape[0], m.data_dim
    out = torch.empty(n, D, device="cuda")
    mask = torch.empty(n, m.mutation_dim, device="cuda")
    sched = dict(sqrt_alphas_cumprod=m.sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod)
    tau = coef = x0c = level = None
    if taus is not None:
        tau, coef = ddim_step_table(m.alphas_cumprod, taus, eta, "sample", **sched)
        x0c = ddim_x0_table(m.alphas_cumprod, tau, eta, "sample", **sched)
        if known is not None:
            level = known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, tau)
    c0 = None if null is None else (C.c_float * len(null))(*null)
    flags = L.OSD_F_GRAPH if m.use_graph else 0
    lo = np.full(D, -np.inf, dtype=np.float32) if lo is None else np.ascontiguousarray(lo, dtype=np.float32)
    hi = np.full(D, np.inf, dtype=np.float32) if hi is None else np.ascontiguousarray(hi, dtype=np.float32)
    rc = L.lib().osd_sample_chain_clipped(eng.handle, L.ptr(cond), n, L.ptr(x_T), L.ptr(zs), seed, row_offset, L.ptr(out), L.ptr(mask), flags,
                                          None if tau is None else tau.ctypes.data, None if coef is None else coef.ctypes.data,
                                          None if x0c is None else x0c.ctypes.data, None if level is None else level.ctypes.data,
                                          0 if tau is None else int(tau.size), c0, w, L.ptr(known), D, lo.ctypes.data, hi.ctypes.data)
    assert rc == expect, (rc, L.last_error())
    torch.cuda.synchronize()
    return out, mask


def chain_link_multistep(m, cond, lo, hi, taus, *, x_T=None, zs=None, seed=0, row_offset=0, known=None, expect=L.OSD_OK):
    """osd_sample_chain_multistep through ctypes on the model's handle with the tables of a sample model: (x_out, mutation mask).
    lo = hi = None are infinite bounds."""
    eng = m._engine()
    n, D = cond.shape[0], m.data_dim
    out = torch.empty(n, D, device="cuda")
    mask = torch.empty(n, m.mutation_dim, device="cuda")
    tau, x0c, hist = dpmpp_2m_table(m.alphas_cumprod, taus, "sample", sqrt_alphas_cumprod=m.sqrt_alphas_cumprod,
                                    sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod)
    level = None if known is None else known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, tau)
    flags = L.OSD_F_GRAPH if m.use_graph else 0
    lo = np.full(D, -np.inf, dtype=np.float32) if lo is None else np.ascontiguousarray(lo, dtype=np.float32)
    hi = np.full(D, np.inf, dtype=np.float32) if hi is None else np.ascontiguousarray(hi, dtype=np.float32)
    rc = L.lib().osd_sample_chain_multistep(eng.handle, L.ptr(cond), n, L.ptr(x_T), L.ptr(zs), seed, row_offset, L.ptr(out), L.ptr(mask), flags,
                                            tau.ctypes.data, x0c.ctypes.data, hist.ctypes.data, None if level is None else level.ctypes.data,
                                            int(tau.size), None, 1.0, L.ptr(known), D, lo.ctypes.data, hi.ctypes.data)
    assert rc == expect, (rc, L.last_error())
    torch.cuda.synchronize()
    return out, mask


def check_link_block(out, mask, md, free=None):
    """Exactly: every link-column value (of the elements `free` selects) in [0, 1]; the mask is (out > 0.5) of the device's own output."""
    blk = out[:, :md]
    inside = (blk >= 0) & (blk <= 1)
    if free is not None:
        inside = inside | ~free[:, :md]
    assert bool(inside.all()), f"{int((~inside).sum())} link-column values outside [0, 1]"
    assert bool(torch.isfinite(out).all())
    assert torch.equal(mask, (blk > 0.5).float())


@pytest.fixture(scope="module")
def case():
    m = ddim_model()
    m.prediction_type, m.mutation_link = "sample", "logistic"
    _use(m, "layers_graph")
    c = make_case(m)
    c["sd64"] = model_sd64(m)
    c["dev"] = dict(cond=c["cond"].cuda(), x_start=c["x_start"].cuda(), zs=c["zs"].cuda())
    return m, c


def _report(tag, out, ref):
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"{tag}: max|ref|={ref.abs().max().item():.3e} tol={tol_of(ref):.3e} err={err:.3e}")
    assert_close(out, ref, RTOL, ATOL, tag)


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_plan_against_fp64_chain(case, eta):
    m, c = case
    d = c["dev"]
    out, mask = chain_link(m, d["cond"], x_T=d["x_start"], zs=d["zs"], taus=PLAN, eta=eta)
    assert L.lib().osd_sample_engine(m._engine().handle, -1, 0) == 0
    ref = chain64(m, c["cond"], c["x_start"], lambda s: c["zs"][len(PLAN) - 1 - s], PLAN, eta, "sample", sd=c["sd64"], out_fn=link_out(MD))
    _report(f"plan eta={eta}", out, ref)
    check_link_block(out, mask, MD)
    # the tolerance separates: the same device output against the chain without the link
    plain = chain64(m, c["cond"], c["x_start"], lambda s: c["zs"][len(PLAN) - 1 - s], PLAN, eta, "sample", sd=c["sd64"])
    assert (out.cpu().double() - plain).abs().max().item() > tol_of(plain)


@pytest.mark.parametrize("mode", ["ddpm", "dpmpp_2m", "guided", "known_bounds"])
def test_sample_options_against_fp64_chain(case, mode):
    m, c = case
    n = 160                                         # two row tiles, the second partial
    g = torch.Generator().manual_seed(43)
    cond = c["cond"][:n].contiguous()
    x_T = torch.randn(n, m.data_dim, generator=g)
    taus = ddim_timesteps(T, S)
    kw, kn, lo, hi = {}, None, None, None
    if mode == "ddpm":                              # the DDPM chain on the short schedule (T = 100)
        zs = torch.randn(T - 1, n, m.data_dim, generator=g)
        ref = chain64(m, cond, x_T, lambda s: zs[T - 1 - s], None, 1.0, "sample", sd=c["sd64"], out_fn=link_out(MD))
    elif mode == "dpmpp_2m":
        zs, kw = None, dict(num_inference_steps=S, solver="dpmpp_2m")
        ref = dpmpp_chain(m, cond, x_T, None, taus, None, None, eps_fn=link_eps_fn(MD), sd=c["sd64"], prediction="sample")
    elif mode == "guided":                          # guidance combines raw outputs: in logit space on the link columns
        zs, kw = torch.randn(S - 1, n, m.data_dim, generator=g), dict(num_inference_steps=S, eta=0.5, guidance_scale=3.0)
        ref = chain64(m, cond, x_T, lambda s: zs[S - 1 - s], taus, 0.5, "sample", sd=c["sd64"], out_fn=link_out(MD, guided_out(3.0, C0_NONZERO)))
    else:                                           # observed values and bounds that cut into the link's range: the clamp follows the link
        zs, kw = torch.randn(S - 1, n, m.data_dim, generator=g), dict(num_inference_steps=S, eta=0.5)
        lo, hi = mixed_bounds()
        lo[:MD], hi[:MD] = 0.45, 0.55
        kn = make_known(c["x0"][:n], "thirty_percent", seed=31)
        kw["known"], kw["x0_bounds"] = kn.cuda(), (lo, hi)
        ref = chain64(m, cond, x_T, lambda s: zs[S - 1 - s], taus, 0.5, "sample", sd=c["sd64"], out_fn=link_out(MD), known=kn, lo=lo, hi=hi)
    if mode == "guided":
        m.null_condition = C0_NONZERO
    try:
        out, mask = m.sample(cond.cuda(), n, x_T=x_T.cuda(), noise=None if zs is None else zs.cuda(), return_mutation_mask=True, **kw)
    finally:
        m.null_condition = None
    assert m.last_sampler == "graph"
    _report(mode, out, ref)
    if kn is None:
        check_link_block(out, mask, MD)
    else:
        obs = ~torch.isnan(kn).cuda()
        assert torch.equal(out[obs], kn.cuda()[obs])                       # observed elements come back bit for bit
        check_link_block(out, mask, MD, free=~obs)
        blk, free = out[:, :MD], ~obs[:, :MD]
        lo_t, hi_t = torch.from_numpy(lo[:MD]).cuda(), torch.from_numpy(hi[:MD]).cuda()
        assert bool((((blk >= lo_t) & (blk <= hi_t)) | ~free).all())                                          # the clamp has the last word
        assert bool((((blk == lo_t) | (blk == hi_t)) & free).any()), "the bounds never cut into the link's range: the case checks nothing"
        assert bool(obs.any()) and bool((~obs).any())


def test_unaligned_dims_on_the_padded_state():
    """dims 62 / 5054 / 26 (D % 4 = 2), n = 16: device-generated draws on the padded state; the link boundary lies inside a quad."""
    dims, cond_dim, n = (62, 5054, 26), 3, 16
    D = sum(dims)
    sd = O.init_state_dict(O.param_shapes(*dims, cond_dim, FULL_H, 128), seed=33)
    conf = config(FULL_H, T=T)
    conf["model"]["diffusion"].update(prediction_type="sample", mutation_link="logistic")
    m = BiologyAwareDiffusionModel(*dims, cond_dim, conf)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.input_splitk = 0
    m.sampler = "graph"
    cond = torch.randn(n, cond_dim, generator=torch.Generator().manual_seed(6))
    seed, off = (7 << 34) + 99, 11
    eng = m._engine()

    def draws(step):
        a = torch.empty(n, D, device="cuda")
        L.check(L.lib().osd_op_randn(eng.handle, L.ptr(a), n, D, seed, off, step, 0))
        return a.cpu()

    noise_T = draws(T)
    zs = {s: draws(s) for s in range(1, len(PLAN))}
    ref = chain64(m, cond, noise_T, lambda s: zs[s], PLAN, 0.5, "sample", out_fn=link_out(dims[0]))
    out, mask = chain_link(m, cond.cuda(), seed=seed, row_offset=off, taus=PLAN, eta=0.5)
    _report(f"padded state D={D}", out, ref)
    check_link_block(out, mask, dims[0])
    # the two columns that share the boundary quad are not linked: against the oracle that links them as well the tolerance is missed
    wider = chain64(m, cond, noise_T, lambda s: zs[s], PLAN, 0.5, "sample", out_fn=link_out(dims[0] + 2))
    assert (out.cpu().double() - wider)[:, dims[0]:dims[0] + 2].abs().max().item() > tol_of(ref)


@pytest.fixture(scope="module")
def philox_case():
    m = ddim_model(seed=2)
    m.prediction_type, m.mutation_link = "sample", "logistic"
    _use(m, "layers_graph")
    cond = torch.randn(N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    return m, cond


def test_rows_do_not_depend_on_chunk_or_shard(philox_case):
    m, cond = philox_case
    kw = dict(seed=13, num_inference_steps=S, eta=0.5, return_mutation_mask=True)
    try:
        whole, whole_mask = m.sample(cond, N, **kw)
        assert m.last_sampler == "graph"
        check_link_block(whole, whole_mask, MD)
        k = 128
        a, ma = m.sample(cond[:k].contiguous(), k, row_offset=0, **kw)
        b, mb = m.sample(cond[k:].contiguous(), N - k, row_offset=k, **kw)
        assert torch.equal(torch.cat([a, b]), whole) and torch.equal(torch.cat([ma, mb]), whole_mask)
        m.sample_chunk_rows = 128
        for engine in ("layers_graph", "layers_eager"):
            _use(m, engine)
            chunked, chunked_mask = m.sample(cond, N, **kw)
            assert torch.equal(chunked, whole) and torch.equal(chunked_mask, whole_mask), engine
    finally:
        _use(m, "layers_graph")
        m.sample_chunk_rows = 65536
        m._engine()
        m.sample_chunk_rows = None


def test_every_engine_setting_routes_to_the_unfolded_steps(philox_case):
    """No x0_bounds, any sampler setting: a linked model runs the per-layer x0-unfolded steps, and its mutation block is inside [0, 1];
    the same model with the identity link leaves the interval."""
    m, cond = philox_case
    try:
        for engine in ("workspace", "squad32", "layers_graph"):
            _use(m, engine)
            for kw in (dict(), dict(num_inference_steps=S), dict(num_inference_steps=S, solver="dpmpp_2m", timestep_spacing="logsnr")):
                out, mask = m.sample(cond, N, seed=21, return_mutation_mask=True, **kw)
                assert m.last_sampler == "graph" and m.last_chain_variant is None, (engine, kw)
                check_link_block(out, mask, MD)
        m.mutation_link = "identity"
        plain = m.sample(cond, N, seed=21, num_inference_steps=S)
        assert not bool(((plain[:, :MD] >= 0) & (plain[:, :MD] <= 1)).all())
    finally:
        m.mutation_link = "logistic"
        _use(m, "layers_graph")


def test_predict_readings(case):
    m, c = case
    g = torch.Generator().manual_seed(21)
    x_t = torch.randn(N, m.data_dim, generator=g).cuda()
    t = torch.randint(0, T, (N,), generator=g).cuda()
    cond = c["dev"]["cond"]
    with torch.no_grad():
        raw = m.predict(x_t, t, cond)
        x0 = m.predict(x_t, t, cond, as_="x0")
        eps = m.predict(x_t, t, cond, as_="eps")
        assert torch.equal(m.predict_noise(x_t, t, cond), eps)
    assert torch.equal(x0[:, MD:], raw[:, MD:])                              # elsewhere: the output, bit for bit
    want = torch.sigmoid(raw[:, :MD].double())
    # fp32 rounding of a value in [0, 1]: the hardware exp2 and rcp (1 ulp each, 2^-23 of sigma <= 1), the rounded exponent argument
    # (|o| 2^-24 sigma' <= |o| 2^-26, |o| < 16 here) and the final rounding: below 8 * 2^-24
    assert float(raw[:, :MD].abs().max()) < 16
    assert (x0[:, :MD].double() - want).abs().max().item() <= 8 * 2.0 ** -24
    assert bool(((x0[:, :MD] >= 0) & (x0[:, :MD] <= 1)).all())
    assert not bool(((raw[:, :MD] >= 0) & (raw[:, :MD] <= 1)).all())          # raw is the logit
    a = m.sqrt_alphas_cumprod[t].view(-1, 1).double()
    b = m.sqrt_one_minus_alphas_cumprod[t].view(-1, 1).double()
    assert_close(a * x0.double() + b * eps.double(), x_t.double(), 1e-5, what="a x0^ + b eps^ against x_t")      # eps^ is derived from the linked x0^


def test_sampling_refusals(philox_case):
    m, cond = philox_case
    eng = m._engine()
    lib = L.lib()
    n, D = 8, m.data_dim
    out = torch.empty(n, D, device="cuda")
    x = torch.randn(n, D, device="cuda")
    with pytest.raises(ValueError, match="mutation_link"):
        m.p_sample(x, 3, cond[:n])
    m.precision = "bf16x3"
    try:
        with pytest.raises(ValueError, match="bf16x3"):
            m.sample(cond[:n], n, num_inference_steps=S)
    finally:
        m.precision = None
    # the library's own refusals: the entry points that fold x0 away
    assert lib.osd_p_sample_step(eng.handle, L.ptr(x), 3, L.ptr(cond[:n]), None, n, 1, 0, L.ptr(out), 0) == L.OSD_EUNSUPPORTED
    assert "osd_set_output_link" in L.last_error()
    assert lib.osd_sample_chain(eng.handle, L.ptr(cond[:n]), n, None, None, 1, 0, L.ptr(out), None, 0) == L.OSD_EUNSUPPORTED
    assert "osd_set_output_link" in L.last_error()
    sched = dict(sqrt_alphas_cumprod=m.sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod)
    tau, coef = ddim_step_table(m.alphas_cumprod, ddim_timesteps(T, S), 0.0, "sample", **sched)
    assert lib.osd_sample_chain_steps(eng.handle, L.ptr(cond[:n]), n, None, None, 1, 0, L.ptr(out), None, 0, tau.ctypes.data, coef.ctypes.data,
                                      int(tau.size)) == L.OSD_EUNSUPPORTED
    m.precision = "bf16x3"                       # the clipped entry point itself refuses the bf16x3 precision
    try:
        chain_link(m, cond[:n], taus=PLAN, expect=L.OSD_EUNSUPPORTED)
    finally:
        m.precision = None
    torch.cuda.synchronize()
    # ... and the handle still samples
    got, mask = chain_link(m, cond[:n], taus=PLAN, seed=3)
    check_link_block(got, mask, MD)
