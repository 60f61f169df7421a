"""GPU: the configurable training loss (l1 / huber / l2, per-timestep weights) of the fused training step against float64 autograd.

The references are torch's own F.l1_loss / F.huber_loss / F.mse_loss in float64 on ``O.training_forward(..., return_loss=False)``
(loss_helpers.Fp64Oracle), at the training tolerances of tests/test_gpu_train_matrix.py: loss 1e-5 relative, each gradient tensor
max|d| <= 5e-5 * max|ref| + 1e-9, and the same bound on the tail columns / rows of input_proj's and output_proj's gradients.  Every
shape's injected noise is first moved off L1's kink (loss_helpers.condition_l1_noise) and then shared by all kinds of that shape, so
one forward graph serves them all.  Each case asserts OSD_TP_LOSS_EPI (include/osdiff.h) and the path bits its shape is there for."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import constraints_oracle as CO
from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import objective as OB
from osteosarcoma_diffusionmodel_amd.train import Trainer, _loss_fwd_bwd
from helpers import RawHandle, assert_close, config
from loss_helpers import (GRAD_RTOL, L1_MARGIN, LOSS_RTOL, P_DROP, SEED, Fp64Oracle, check, condition_l1_noise, inputs, philox_masks,
                          predict_fp64)

pytestmark = pytest.mark.gpu

SQ_FWD, XPAD, MSE_BF16, LOSS_EPI = 1 << 0, 1 << 6, 1 << 10, 1 << 11      # include/osdiff.h: OSD_TP_*
REAL = (62, 5054, 26, 4)        # D = 5142, D % 4 == 2: the guarded epilogue and a ragged feature tile
FULL = (50, 1900, 50, 3)        # D = 2000: the transposer (FAST) path
DEEP = (16, 480, 16, 3)
H3 = [256, 512, 256]
H4 = [256, 256, 512, 256]
LR, WD = 1e-4, 1e-5

# shape groups: dims, hidden, rows, how the keep-masks are drawn
SHAPES = {
    "real16": dict(dims=REAL, hidden=H3, n=16, draw="injected"),
    "real16-eval": dict(dims=REAL, hidden=H3, n=16, draw="eval"),
    "full2111": dict(dims=FULL, hidden=H3, n=2111, draw="philox"),
    "deep300": dict(dims=DEEP, hidden=H4, n=300, draw="philox"),
}
_cache = {}


def _min_snr(gamma=5.0):
    return OB.min_snr_weights(O.schedule_buffers("cosine", 1000)["alphas_cumprod"], gamma)


def _custom_table():
    return torch.rand(1000, generator=torch.Generator().manual_seed(4)) * 2 + 0.05      # random, positive


def _shape(name):
    """Inputs of a shape group with the noise conditioned for L1, and the group's fp64 forward graph (built once, left unchanged)."""
    if name not in _cache:
        s = SHAPES[name]
        sd, x, cond, t, noise, injected = inputs(s["dims"], s["hidden"], s["n"])
        masks = {"injected": injected, "philox": None, "eval": None}[s["draw"]]
        if s["draw"] == "philox":
            masks = philox_masks(s["hidden"], s["n"])
        noise, counts = condition_l1_noise(lambda nz: predict_fp64(sd, x, cond, t, nz, s["hidden"], masks, P_DROP), noise)
        print(f"[{name}] residuals inside the L1 margin, round by round: {counts}")
        assert counts[-1] == 0, f"{name}: {counts[-1]} residuals are still within {L1_MARGIN} of L1's kink after {len(counts) - 1} rounds"
        orc = Fp64Oracle(sd, x, cond, t, noise, s["hidden"], masks, P_DROP)
        assert float((orc.pred.detach() - noise.double()).abs().min()) >= L1_MARGIN
        _cache[name] = (sd, x, cond, t, noise, injected, orc)
    return _cache[name]


def _model(name, sd, precision=None, **diffusion):
    s = SHAPES[name]
    mut, expr, pw, cd = s["dims"]
    conf = config(s["hidden"], p=P_DROP)
    conf["model"]["diffusion"].update(diffusion)
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda()
    m = m.eval() if s["draw"] == "eval" else m.train()
    m.precision = precision
    return m


def _path(m):
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(m._engine().handle, b"last_train_path", C.byref(v)))
    return int(v.value)


def _run(name, m, with_grads=True, loss_scale=1.0):
    """(loss, {name: gradient} or None, last_train_path) of one training call of ``m`` on the shape group's inputs."""
    s = SHAPES[name]
    sd, x, cond, t, noise, injected, _ = _shape(name)
    grads = [torch.empty_like(p) for p in m.parameters()] if with_grads else None
    kw = dict(t=t.cuda(), noise=noise.cuda(), seed=SEED, loss_scale=loss_scale)
    if s["draw"] == "injected":
        kw["dropout_masks"] = [k.cuda() for k in injected]
    loss = _loss_fwd_bwd(m, x.cuda(), cond.cuda(), None if grads is None else L.ptr_array(grads), **kw)
    torch.cuda.synchronize()
    names = [k for k, _ in m.named_parameters()]
    return loss.item(), None if grads is None else {k: g.cpu() for k, g in zip(names, grads)}, _path(m)


def _compare(name, tag, got, ref):
    loss, grads, _ = got
    worst, bad = check(loss, grads, ref[0], ref[1], sum(SHAPES[name]["dims"][:3]))
    print(f"[{name} {tag}] loss {loss:.8g} (fp64 {ref[0]:.8g}); worst error / tolerance {worst:.3f}")
    return bad


# (shape group, loss_type, huber_delta, weighting: None | "min_snr" | "custom", precision, path bits set, path bits clear)
CASES = {
    "real16-l1": ("real16", "l1", 1.0, None, None, 0, SQ_FWD | MSE_BF16),
    "real16-huber": ("real16", "huber", 1.0, None, None, 0, SQ_FWD | MSE_BF16),
    "real16-huber0.3-minsnr": ("real16", "huber", 0.3, "min_snr", None, 0, SQ_FWD | MSE_BF16),
    "real16-l2-minsnr": ("real16", "l2", 1.0, "min_snr", None, 0, SQ_FWD | MSE_BF16),
    "full2111-l1-minsnr": ("full2111", "l1", 1.0, "min_snr", None, SQ_FWD | XPAD, MSE_BF16),
    "full2111-huber": ("full2111", "huber", 1.0, None, None, SQ_FWD | XPAD, MSE_BF16),
    "deep300-huber-custom": ("deep300", "huber", 1.0, "custom", None, 0, SQ_FWD | MSE_BF16),
    # bf16x3: launch_loss_b3t takes any row count (its preconditions are alignment and D % 4 == 0), so the smallest interesting one is
    # the 2 111 rows whose oracle is already there: 128 x 128 tiles (>= 256 of them) and a ragged last row block
    "full2111-b3-huber-minsnr": ("full2111", "huber", 1.0, "min_snr", "bf16x3", SQ_FWD | XPAD | MSE_BF16, 0),
}


def _weights(weighting):
    return {None: None, "min_snr": _min_snr(), "custom": _custom_table()}[weighting]


def _device(case):
    if ("dev", case) not in _cache:
        name, kind, delta, weighting, precision, _, _ = CASES[case]
        sd = _shape(name)[0]
        m = _model(name, sd, precision, loss_type=kind, huber_delta=delta, loss_weighting="min_snr" if weighting == "min_snr" else None)
        if weighting == "custom":
            m.set_loss_weights(_custom_table())
        _cache[("dev", case)] = _run(name, m)
    return _cache[("dev", case)]


def _reference(case):
    if ("ref", case) not in _cache:
        name, kind, delta, weighting, _, _, _ = CASES[case]
        _cache[("ref", case)] = _shape(name)[6].loss_and_grads(kind, delta, _weights(weighting))
    return _cache[("ref", case)]


@pytest.mark.parametrize("case", list(CASES))
def test_loss_kinds_vs_fp64_autograd(case):
    """Cases 1-4: loss, every gradient and the tail slices; OSD_TP_LOSS_EPI and the path bits of the shape."""
    name, kind, delta, weighting, _, want_set, want_clear = CASES[case]
    got = _device(case)
    bad = _compare(name, case, got, _reference(case))
    assert not bad, "\n".join(bad)
    path = got[2]
    assert path & LOSS_EPI, f"last_train_path {path:#x}: the loss epilogue did not run"
    assert path & want_set == want_set and not path & want_clear, f"last_train_path {path:#x}, wanted {want_set:#x} set and {want_clear:#x} clear"
    if kind == "huber" and delta == 0.3:
        d = (_shape(name)[6].pred.detach() - _shape(name)[4].double()).abs()
        assert int((d <= delta).sum()) > 1000 and int((d > delta).sum()) > 1000      # both branches of rho are populated


def test_loss_only_call_gives_the_same_loss():
    """Case 5: eval mode at case 1's shape, grads = None (validation) against the call with gradients and against the oracle.  The two
    device values come from the same launches; their float atomics may land in another order, which moves the sum of a few hundred
    partials by a few ulp: 1e-6 relative."""
    name = "real16-eval"
    sd = _shape(name)[0]
    ref = _shape(name)[6].loss_and_grads("huber", 0.3, _min_snr())
    m = _model(name, sd, loss_type="huber", huber_delta=0.3, loss_weighting="min_snr")
    with_g = _run(name, m)
    assert not _compare(name, "huber0.3-minsnr with gradients", with_g, ref)
    only, none, path = _run(name, m, with_grads=False)
    print(f"[{name}] loss only {only:.9g}, with gradients {with_g[0]:.9g}")
    assert none is None and path & LOSS_EPI
    assert_close(only, ref[0], LOSS_RTOL, what="loss-only call vs fp64")
    assert_close(only, with_g[0], 1e-6, what="loss-only call vs the call with gradients")


def test_constraints_on_top_of_huber_vs_fp64_autograd():
    """Case 6: set_constraints + huber at dims (16, 224, 16, 3), 256 rows, eval mode, against fp64 autograd of the composite at the
    tolerances of tests/test_gpu_constraints.py (totals and parts 2e-5, gradients 1e-4 * max|ref| + 1e-9); parts[0] is the Huber part."""
    dims, hidden, n, delta = (16, 224, 16, 3), H3, 256, 0.8
    sd, x0, cond, t, noise, _ = inputs(dims, hidden, n)
    mut, expr, pwd, cd = dims
    D = mut + expr + pwd
    pw = [[mut + 1, mut + 7, mut + 100, mut + 201], [mut + 3, mut + expr - 1, D - 2], [mut + 5, mut + 6, mut + 9, D - 1]]
    ca, cb = list(range(0, 16)), list(range(mut + expr - 16, mut + expr))
    w_pc, w_me = 0.7, 1.3
    orc = Fp64Oracle(sd, x0, cond, t, noise, hidden)
    parts = {}

    def composite(pred):
        hub = orc.eps_loss(pred, "huber", delta)
        x_t = O.q_sample(orc.bufs, x0.double(), t, noise.double())
        xh = CO.x0_hat(x_t, pred, t, orc.bufs["sqrt_alphas_cumprod"], orc.bufs["sqrt_one_minus_alphas_cumprod"])
        l_pc = CO.pathway_coherence_loss(xh, pw)
        l_me = CO.mutation_expression_correlation_loss(xh, x0.double(), ca, cb)
        parts.update(hub=hub.item(), pc=l_pc.item(), me=l_me.item())
        return hub + w_pc * l_pc + w_me * l_me

    total, ref = orc.grads_of(composite)
    conf = config(hidden, p=P_DROP)
    conf["model"]["diffusion"].update(loss_type="huber", huber_delta=delta)
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pwd, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.set_constraints(pw, ca, cb, pathway_weight=w_pc, mutexpr_weight=w_me)
    loss = m(x0.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda())
    loss.backward()
    path = _path(m)
    got = m.last_loss_parts()
    print(f"[cons] total {loss.item():.8g} (fp64 {total:.8g}); parts {got} (fp64 {parts})")
    assert_close(loss.item(), total, 2e-5, what="total loss")
    assert_close(got[0], parts["hub"], 2e-5, what="huber part")
    assert_close(got[1], parts["pc"], 2e-5, atol=1e-7, what="L_pc part")
    assert_close(got[2], parts["me"], 2e-5, atol=1e-7, what="L_me part")
    assert abs(parts["hub"] - torch.nn.functional.mse_loss(orc.pred.detach(), noise.double()).item()) > 1e-2 * parts["hub"]   # not the MSE
    named = dict(m.named_parameters())
    for k, gr in ref.items():
        assert_close(named[k].grad.cpu(), gr, 1e-4, atol=1e-9, what=f"grad {k}")
    assert path & LOSS_EPI, f"last_train_path {path:#x}"


# ---- case 7: the Trainer ------------------------------------------------------------------------------------------------------
def _train_conf(hidden, tmp_path, **diffusion):
    conf = config(hidden, p=P_DROP)
    conf["model"]["diffusion"].update(diffusion)
    conf["training"] = {"learning_rate": LR, "weight_decay": WD, "patience": 10, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.0},
                        "save_dir": str(tmp_path), "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": 16}
    return conf


def _assert_params_close(got, want, gclip, name):
    """tests/test_gpu_train_matrix.py's rule: 2e-5 * max|p| plus the gradient tolerance propagated through the first AdamW update (steep
    where the clipped gradient is comparable to eps = 1e-8), never more than the 2 lr of a flipped sign."""
    got, want, g = got.double().numpy(), want.double().numpy(), np.abs(gclip.double().numpy())
    d = np.abs(got - want)
    assert np.isfinite(got).all(), name
    eps = 1e-8
    sens = LR * eps / (g + eps) ** 2
    allowed = 2e-5 * np.abs(want).max() + 1e-8 + np.minimum(sens * GRAD_RTOL * g.max(), 2.0 * LR)
    worst = (d - allowed).max()
    assert worst <= 0, f"param {name}: an element exceeds its propagated tolerance by {worst:.3e} (max|d|={d.max():.3e})"


def _trainer_model(conf):
    mut, expr, pw, cd = REAL
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(_shape("real16")[0], strict=False)
    return m.cuda().train()


def _step_reference(ref_grads, sd):
    names = list(sd)
    clipped, norm = O.clip_grad_norm([ref_grads[k] for k in names], 1.0)
    p1 = [sd[k].double().clone() for k in names]
    m1 = [torch.zeros_like(v) for v in p1]
    v1 = [torch.zeros_like(v) for v in p1]
    O.adamw_step(p1, clipped, m1, v1, 1, lr=LR, weight_decay=WD)
    return names, clipped, norm, p1


def _check_step(tr, m, loss, ref_loss, ref_grads, sd):
    names, clipped, norm, p1 = _step_reference(ref_grads, sd)
    assert_close(loss.item(), ref_loss, LOSS_RTOL, what="train_step loss")
    assert_close(tr.optimizer.grad_norm.item(), norm.item(), 2e-5, what="pre-clip gradient norm")
    assert _path(m) & LOSS_EPI
    for k, p in m.named_parameters():
        j = names.index(k)
        _assert_params_close(p.detach().cpu(), p1[j], clipped[j], k)


def test_trainer_step_and_validate_use_the_configured_loss(tmp_path, monkeypatch):
    """One Trainer.train_step with loss_type: huber, loss_weighting: min_snr in the config against O.clip_grad_norm + O.adamw_step on the
    fp64 gradients; Trainer.validate (resident rows, eval mode, t / noise injected into its calls) returns the configured loss."""
    from osteosarcoma_diffusionmodel_amd import train as T
    from osteosarcoma_diffusionmodel_amd.train import OsteosarcomaDataset
    sd, x, cond, t, noise, injected, orc = _shape("real16")
    ref_loss, ref_grads = orc.loss_and_grads("huber", 1.0, _min_snr())
    conf = _train_conf(H3, tmp_path, loss_type="huber", loss_weighting="min_snr")
    m = _trainer_model(conf)
    ds = object.__new__(OsteosarcomaDataset)
    ds.data, ds.conditions, ds.survival_days = x.clone(), cond.clone(), torch.rand(16) * 1000
    loader = torch.utils.data.DataLoader(ds, batch_size=16, shuffle=False, num_workers=0)
    tr = Trainer(m, loader, loader, conf, device="cuda")
    # validate first (it leaves the parameters alone): eval mode, so its own oracle
    ev = _shape("real16-eval")
    assert torch.equal(ev[1], x) and torch.equal(ev[3], t)
    val_ref, _ = ev[6].loss_and_grads("huber", 1.0, _min_snr())
    mse_ref, _ = ev[6].loss_and_grads("l2")
    orig, calls = T._loss_fwd_bwd, []

    def injected_draws(*a, **k):
        calls.append(k.get("source") is not None)
        return orig(*a, t=t.cuda(), noise=ev[4].cuda(), **k)

    monkeypatch.setattr(T, "_loss_fwd_bwd", injected_draws)
    val = tr.validate()
    monkeypatch.setattr(T, "_loss_fwd_bwd", orig)
    print(f"[trainer] validate {val:.8g} (fp64 huber + min-SNR {val_ref:.8g}, fp64 mse {mse_ref:.8g})")
    assert calls == [True] and tr.resident                       # one batch, taken from the resident dataset
    assert_close(val, val_ref, LOSS_RTOL, what="validate")
    assert abs(val_ref - mse_ref) > 1e-2 * mse_ref               # the MSE would not have passed
    m.train()
    loss = tr.train_step(x.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in injected])
    _check_step(tr, m, loss, ref_loss, ref_grads, sd)


def test_trainer_follows_a_loss_changed_after_construction(tmp_path):
    """The Trainer's fast path keeps its engine: model.loss_type / loss_weighting assigned after construction reach the next step."""
    sd, x, cond, t, noise, injected, orc = _shape("real16")
    conf = _train_conf(H3, tmp_path)
    m = _trainer_model(conf)
    tr = Trainer(m, [], [], conf, device="cuda")
    m.loss_type, m.loss_weighting = "l1", "min_snr"
    ref_loss, ref_grads = orc.loss_and_grads("l1", 1.0, _min_snr())
    loss = tr.train_step(x.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in injected])
    _check_step(tr, m, loss, ref_loss, ref_grads, sd)
    m.loss_type = "cauchy"
    with pytest.raises(ValueError):
        tr.train_step(x.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in injected])


def test_loss_scale_halves_the_gradients_not_the_loss():
    """Data parallel hands loss_scale = 1 / world: at 0.5 every gradient is half (gscale halves exactly; the sums that follow may be
    taken in another order, so the gradient tolerance, not bits) and the loss is the unscaled one."""
    name = "real16"
    full = _device("real16-huber0.3-minsnr")
    m = _model(name, _shape(name)[0], loss_type="huber", huber_delta=0.3, loss_weighting="min_snr")
    half = _run(name, m, loss_scale=0.5)
    assert_close(half[0], full[0], 1e-6, what="loss under loss_scale = 0.5")
    bad = _compare(name, "loss_scale 0.5, gradients doubled", (half[0], {k: 2 * g for k, g in half[1].items()}, 0), _reference("real16-huber0.3-minsnr"))
    assert not bad, "\n".join(bad)
    for k in full[1]:
        assert_close(2 * half[1][k], full[1][k], GRAD_RTOL, atol=1e-9, what=f"2 x grad {k} at loss_scale 0.5")


# ---- case 8: the default is untouched ---------------------------------------------------------------------------------------------
def test_default_path_is_unchanged_and_l2_with_ones_agrees():
    """A config without the keys and one that says loss_type: l2 run the same kernels: equal bits, OSD_TP_LOSS_EPI absent.  The shape is
    one whose training step is reproducible run to run (a single output_proj workgroup in which one wave holds every valid row, so the
    loss is one non-zero partial; block widths whose GroupNorm backward reduces in a fixed order): first shown on the default model
    itself.  l2 with an all-ones table runs the new epilogue and agrees with the default within the training tolerances."""
    dims, hidden, n = (8, 24, 8, 3), [32, 64, 32], 16
    sd, x, cond, t, noise, injected = inputs(dims, hidden, n)
    mut, expr, pw, cd = dims

    def run(table=None, **diffusion):
        conf = config(hidden, p=P_DROP)
        conf["model"]["diffusion"].update(diffusion)
        m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
        m.load_state_dict(sd, strict=False)
        m = m.cuda().train()
        if table is not None:
            m.set_loss_weights(table)
        grads = [torch.empty_like(p) for p in m.parameters()]
        loss = _loss_fwd_bwd(m, x.cuda(), cond.cuda(), L.ptr_array(grads), t=t.cuda(), noise=noise.cuda(), seed=SEED,
                             dropout_masks=[k.cuda() for k in injected])
        torch.cuda.synchronize()
        return loss.cpu(), {k: g.cpu() for (k, _), g in zip(m.named_parameters(), grads)}, _path(m)

    base, again, named = run(), run(), run(loss_type="l2", loss_weighting=None)
    assert torch.equal(base[0], again[0]) and all(torch.equal(base[1][k], again[1][k]) for k in base[1]), "the default step is not reproducible here"
    assert torch.equal(base[0], named[0]), (base[0], named[0])
    for k in base[1]:
        assert torch.equal(base[1][k], named[1][k]), k
    assert not base[2] & LOSS_EPI and not named[2] & LOSS_EPI and base[2] == named[2]
    ones = run(table=torch.ones(1000), loss_type="l2")
    assert ones[2] & LOSS_EPI and ones[2] & ~LOSS_EPI == base[2]
    worst, bad = check(ones[0].item(), ones[1], base[0].item(), base[1], mut + expr + pw)
    print(f"[default] l2 + all-ones table vs the default: worst error / tolerance {worst:.3f}")
    assert not bad, "\n".join(bad)


# ---- case 9: negative controls ----------------------------------------------------------------------------------------------------
def _misses(case, ref):
    name = CASES[case][0]
    return _compare(name, f"{case} (negative control)", _device(case), ref)


def test_negative_control_huber_delta():
    """Device huber at delta = 1 against the oracle at delta = 1.05."""
    assert _misses("real16-huber", _shape("real16")[6].loss_and_grads("huber", 1.05)), "a wrong delta went unnoticed"


def test_negative_control_weights_left_out():
    """min-SNR on the device against the unweighted oracle."""
    assert _misses("real16-l2-minsnr", _shape("real16")[6].loss_and_grads("l2")), "missing weights went unnoticed"


def test_negative_control_table_shifted_by_one_timestep():
    """min-SNR on the device against the oracle with w[t + 1] in place of w[t]."""
    w = _min_snr()
    shifted = torch.cat([w[1:], w[-1:]])
    assert _misses("real16-l2-minsnr", _shape("real16")[6].loss_and_grads("l2", 1.0, shifted)), "a shifted table went unnoticed"


def test_negative_control_l1_against_l2():
    assert _misses("real16-l1", _shape("real16")[6].loss_and_grads("l2")), "the wrong kind went unnoticed"


# ---- case 10: errors --------------------------------------------------------------------------------------------------------------
def test_bad_settings_raise_value_error():
    name = "real16"
    sd = _shape(name)[0]
    with pytest.raises(ValueError):
        _model(name, sd, loss_type="cauchy")
    for delta in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _model(name, sd, loss_type="huber", huber_delta=delta)
    m = _model(name, sd)
    for table in (torch.ones(999), -torch.ones(1000), torch.full((1000,), float("nan"))):
        with pytest.raises(ValueError):
            m.set_loss_weights(table)
    # assigned after construction: the next training call raises, and the handle keeps the setting it had
    for attr, value in (("loss_type", "cauchy"), ("huber_delta", 0.0), ("huber_delta", float("inf")), ("loss_weighting", "snr")):
        keep = getattr(m, attr)
        setattr(m, attr, value)
        with pytest.raises(ValueError):
            _run(name, m, with_grads=False)
        setattr(m, attr, keep)
    loss, _, path = _run(name, m, with_grads=False)
    assert np.isfinite(loss) and not path & LOSS_EPI


def test_osd_set_loss_rejects_bad_arguments():
    """The C entry point: OSD_EINVAL and a message for an unknown kind, delta <= 0 or non-finite, a negative or NaN weight; the table has
    T entries (RawHandle: T = 10)."""
    rh = RawHandle()
    try:
        lib = L.lib()
        good = np.ones(10, dtype=np.float32)

        def call(kind, delta, table):
            return lib.osd_set_loss(rh.h, kind, delta, None if table is None else table.ctypes.data)

        assert call(L.OSD_LOSS_HUBER, 0.5, good) == L.OSD_OK and call(L.OSD_LOSS_L1, 1.0, None) == L.OSD_OK
        neg, nan, inf = good.copy(), good.copy(), good.copy()
        neg[3], nan[9], inf[0] = -1e-3, np.nan, np.inf
        for kind, delta, table in ((3, 1.0, None), (-1, 1.0, None), (L.OSD_LOSS_HUBER, 0.0, None), (L.OSD_LOSS_HUBER, -2.0, None),
                                   (L.OSD_LOSS_HUBER, float("nan"), None), (L.OSD_LOSS_L2, float("inf"), None), (L.OSD_LOSS_L2, 1.0, neg),
                                   (L.OSD_LOSS_L2, 1.0, nan), (L.OSD_LOSS_L1, 1.0, inf)):
            assert call(kind, delta, table) == L.OSD_EINVAL, (kind, delta)
            assert L.last_error(), "no message"
        assert call(L.OSD_LOSS_L2, 1.0, None) == L.OSD_OK
    finally:
        rh.close()
