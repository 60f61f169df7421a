"""GPU: training on incomplete patients -- the NaN-masked q_sample prologue and loss epilogue of the fused training step (DESIGN.md
section 3.23) against float64 autograd (mask_helpers.MaskedOracle on loss_helpers.Fp64Oracle).

Shapes are those of tests/test_gpu_loss.py, the missing-value pattern is mask_helpers.mask_pattern (its properties are asserted in
tests/test_mask_cpu.py), tolerances are the project's training tolerances: loss 1e-5 relative, each gradient tensor
max|d| <= 5e-5 * max|ref| + 1e-9 and the same bound on the tail columns / rows of input_proj's and output_proj's gradients
(loss_helpers.check).  The injected noise of real16 / deep300 is moved off L1's kink on the zero-filled input
(loss_helpers.condition_l1_noise); at full2111, whose L1 case predicts x0, it is x0 that is moved (mask_helpers.condition_l1_x0: there
d = out - x0 does not contain the noise) and every case of the shape shares that input and one forward graph."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd import objective as OB
from osteosarcoma_diffusionmodel_amd.train import MixupAugmentation, OsteosarcomaDataset, Trainer, _loss_fwd_bwd
from helpers import assert_close, config
from loss_helpers import GRAD_RTOL, L1_MARGIN, LOSS_RTOL, P_DROP, SEED, Fp64Oracle, check, condition_l1_noise, inputs, philox_masks, predict_fp64
from mask_helpers import (DEEP, FULL, H3, H4, PROLOGUE_SHAPES, SHAPES, MaskedOracle, MixupMaskedOracle, condition_l1_x0, mask_pattern,
                          q_sample_fp32, with_nan, zero_fill)

pytestmark = pytest.mark.gpu

SQ_FWD, XPAD, MSE_BF16, LOSS_EPI, MASKED = 1 << 0, 1 << 6, 1 << 10, 1 << 11, 1 << 14      # include/osdiff.h: OSD_TP_*
LR, WD = 1e-4, 1e-5
_cache = {}


def _weights(weighting, prediction):
    if weighting == "min_snr":
        return OB.min_snr_weights(O.schedule_buffers("cosine", 1000)["alphas_cumprod"], 5.0, prediction)
    if weighting == "custom":
        return torch.rand(1000, generator=torch.Generator().manual_seed(4)) * 2 + 0.05
    return None


def _shape(name):
    """(sd, x with NaN, cond, t, noise, injected masks, oracle) of a shape group: built once, left unchanged."""
    if name not in _cache:
        s = SHAPES[name]
        sd, x, cond, t, noise, injected = inputs(s["dims"], s["hidden"], s["n"])
        masks = injected if s["draw"] == "injected" else philox_masks(s["hidden"], s["n"])
        x = with_nan(x, mask_pattern(s["n"], s["dims"]))
        if name == "full2111":
            x, counts = condition_l1_x0(lambda xf: predict_fp64(sd, xf, cond, t, noise, s["hidden"], masks, P_DROP), x)
        else:
            noise, counts = condition_l1_noise(lambda nz: predict_fp64(sd, zero_fill(x), cond, t, nz, s["hidden"], masks, P_DROP), noise)
        print(f"[{name}] residuals inside the L1 margin, round by round: {counts}")
        assert counts[-1] == 0, f"{name}: {counts[-1]} residuals are still within {L1_MARGIN} of L1's kink"
        orc = MaskedOracle(sd, x, cond, t, noise, s["hidden"], masks, P_DROP)
        _cache[name] = (sd, x, cond, t, noise, injected, orc)
    return _cache[name]


def _model(name, sd, precision=None, missing_values="mask", **diffusion):
    s = SHAPES[name]
    mut, expr, pw, cd = s["dims"]
    conf = config(s["hidden"], p=P_DROP)
    conf["model"]["diffusion"].update(diffusion)
    if missing_values is not None:
        conf["training"] = {"missing_values": missing_values}
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    m.precision = precision
    return m


def _path(m):
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(m._engine().handle, b"last_train_path", C.byref(v)))
    return int(v.value)


def _run(name, m, x=None, cond=None, source=None, with_grads=True):
    """(loss, {name: gradient} or None, last_train_path) of one training call of ``m`` with the shape group's t / noise / masks."""
    s = SHAPES[name]
    sd, x_nan, cond0, t, noise, injected, _ = _shape(name)
    grads = [torch.empty_like(p) for p in m.parameters()] if with_grads else None
    kw = dict(t=t.cuda(), noise=noise.cuda(), seed=SEED)
    if s["draw"] == "injected":
        kw["dropout_masks"] = [k.cuda() for k in injected]
    if source is not None:
        loss = _loss_fwd_bwd(m, None, None, None if grads is None else L.ptr_array(grads), source=source, **kw)
    else:
        loss = _loss_fwd_bwd(m, (x_nan if x is None else x).cuda(), (cond0 if cond is None else cond).cuda(),
                             None if grads is None else L.ptr_array(grads), **kw)
    torch.cuda.synchronize()
    names = [k for k, _ in m.named_parameters()]
    return loss.item(), None if grads is None else {k: g.cpu() for k, g in zip(names, grads)}, _path(m)


def _compare(name, tag, got, ref):
    worst, bad = check(got[0], got[1], ref[0], ref[1], sum(SHAPES[name]["dims"][:3]), show=tag)
    print(f"[{name} {tag}] loss {got[0]:.8g} (fp64 {ref[0]:.8g}); worst error / tolerance {worst:.3f}")
    return bad


# ---- case 1: the prologue, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("shape", list(PROLOGUE_SHAPES))
def test_prologue_bits(shape, prediction):
    """osd_q_sample_target under the mask, injected t and noise: x_t has the bits of the host fp32 restatement on the zero-filled input,
    the target is NaN exactly where x0 is, and elsewhere has the bits the unmasked call returns for the zero-filled input."""
    dims, n = PROLOGUE_SHAPES[shape]
    sd, x, cond, t, noise, _ = inputs(dims, H3, n)
    miss = mask_pattern(n, dims)
    x = with_nan(x, miss)
    mut, expr, pw, cd = dims
    m = BiologyAwareDiffusionModel(config=config(H3, p=P_DROP), mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd).cuda()
    m.prediction_type = prediction
    m.missing_values = "mask"
    x_t, target = m.q_sample(x.cuda(), t.cuda(), noise.cuda(), return_target=True)
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(m._engine().handle, b"loss_mask", C.byref(v)))
    assert v.value == 1
    m.missing_values = None
    x_t0, target0 = m.q_sample(zero_fill(x).cuda(), t.cuda(), noise.cuda(), return_target=True)
    L.check(L.lib().osd_get_option(m._engine().handle, b"loss_mask", C.byref(v)))
    assert v.value == 0
    x_t, target, x_t0, target0 = x_t.cpu(), target.cpu(), x_t0.cpu(), target0.cpu()
    bufs = {k: getattr(m, k).detach().cpu() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
    host_xt, host_target = q_sample_fp32(x, t, noise, prediction, bufs)
    assert torch.isfinite(x_t).all()
    assert torch.equal(x_t.view(torch.int32), host_xt.view(torch.int32)), "x_t differs from the host fp32 restatement"
    assert torch.equal(x_t.view(torch.int32), x_t0.view(torch.int32))
    assert torch.equal(torch.isnan(target), miss), "the target's NaN are not x0's"
    assert torch.isfinite(target0).all()
    assert torch.equal(target[~miss].view(torch.int32), target0[~miss].view(torch.int32)), "observed target elements differ from the unmasked call"
    assert torch.equal(target[~miss].view(torch.int32), host_target[~miss].view(torch.int32))


# ---- case 2: loss and every gradient against the fp64 oracle ------------------------------------------------------------------------
# (shape group, loss_type, huber_delta, weighting, prediction_type, path bits set, path bits clear)
CASES = {
    "real16-l2-eps": ("real16", "l2", 1.0, None, "epsilon", 0, SQ_FWD | XPAD | MSE_BF16),
    "real16-huber0.3-minsnr-v": ("real16", "huber", 0.3, "min_snr", "v_prediction", 0, SQ_FWD | XPAD | MSE_BF16),
    "full2111-l2-eps": ("full2111", "l2", 1.0, None, "epsilon", SQ_FWD | XPAD, MSE_BF16),
    "full2111-l1-minsnr-sample": ("full2111", "l1", 1.0, "min_snr", "sample", SQ_FWD | XPAD, MSE_BF16),
    "deep300-huber-custom": ("deep300", "huber", 1.0, "custom", "epsilon", 0, SQ_FWD | XPAD | MSE_BF16),
}


def _reference(case):
    if ("ref", case) not in _cache:
        name, kind, delta, weighting, prediction, _, _ = CASES[case]
        _cache[("ref", case)] = _shape(name)[6].loss_and_grads(kind, delta, _weights(weighting, prediction), prediction)
    return _cache[("ref", case)]


def _case_model(case, precision=None):
    name, kind, delta, weighting, prediction, _, _ = CASES[case]
    m = _model(name, _shape(name)[0], precision, loss_type=kind, huber_delta=delta, prediction_type=prediction,
               loss_weighting="min_snr" if weighting == "min_snr" else None)
    if weighting == "custom":
        m.set_loss_weights(_weights("custom", prediction))
    return m


@pytest.mark.parametrize("case", list(CASES))
def test_masked_loss_vs_fp64_autograd(case):
    name, kind, delta, weighting, prediction, want_set, want_clear = CASES[case]
    ref = _reference(case)
    if kind == "l1":
        orc = _shape(name)[6]
        d = (orc.pred.detach() - zero_fill(orc.inner.x0)).abs()
        assert float(d[orc.observed].min()) >= L1_MARGIN
    got = _run(name, _case_model(case))
    bad = _compare(name, case, got, ref)
    assert not bad, "\n".join(bad)
    path = got[2]
    assert path & MASKED, f"last_train_path {path:#x}: the masked path did not run"
    assert path & want_set == want_set and not path & want_clear, f"last_train_path {path:#x}, wanted {want_set:#x} set and {want_clear:#x} clear"
    assert ref[0] > 0 and np.isfinite(got[0])


def test_negative_control_mask_left_out_of_the_oracle():
    """The device's masked loss against the oracle of the zero-filled input WITHOUT the mask: must miss."""
    name = "real16"
    sd, x, cond, t, noise, injected, orc = _shape(name)
    unmasked = orc.inner.loss_and_grads("l2")
    assert _compare(name, "negative control", _run(name, _case_model("real16-l2-eps")), unmasked), "a missing mask went unnoticed"


# ---- case 3: resident source with mixup ---------------------------------------------------------------------------------------------
def test_resident_source_with_mixup():
    """osd_train_batch_source with idx_b set, lam = 0.3, at deep300: against the mixup oracle; then the same rows as a plain batch after
    the Trainer's own mix (MixupAugmentation.mix, which propagates NaN alike), against the same oracle and tolerance."""
    name, lam = "deep300", 0.3
    sd, x, cond, t, noise, injected, _ = _shape(name)
    n = SHAPES[name]["n"]
    g = torch.Generator().manual_seed(11)
    idx_a, perm = torch.randperm(n, generator=g), torch.randperm(n, generator=g)
    idx_b = idx_a[perm]
    orc = MixupMaskedOracle(sd, x, cond, idx_a, idx_b, lam, t, noise, H4, philox_masks(H4, n), P_DROP)
    both = int((~orc.observed).sum()) - int(torch.isnan(x[idx_a]).sum())
    assert both > 0, "no element is missing through the second parent alone"
    ref = orc.loss_and_grads("l2")
    m = _model(name, sd)
    data, conds = x.cuda(), cond.cuda()
    got = _run(name, m, source=(data, conds, idx_a.cuda(), idx_b.cuda(), lam))
    bad = _compare(name, "resident source + mixup", got, ref)
    assert not bad, "\n".join(bad)
    assert got[2] & MASKED and got[2] & LOSS_EPI
    mixed = MixupAugmentation(alpha=0.2).mix({"data": data[idx_a.cuda()], "conditions": conds[idx_a.cuda()], "survival": torch.zeros(n).cuda()},
                                             lam, perm.cuda())
    assert torch.equal(torch.isnan(mixed["data"]).cpu(), ~orc.observed)
    assert torch.equal(zero_fill(mixed["data"]).cpu(), zero_fill(orc.x_mix))
    plain = _run(name, m, x=mixed["data"], cond=mixed["conditions"])
    bad = _compare(name, "plain batch after a host-side mix", plain, ref)
    assert not bad, "\n".join(bad)
    assert plain[2] & MASKED


# ---- case 4: mask on, all-finite batch ------------------------------------------------------------------------------------------------
def test_mask_on_all_finite_batch_agrees_with_the_unmasked_call():
    name = "real16"
    sd, x, cond, t, noise, injected, _ = _shape(name)
    xf = zero_fill(x)
    for diffusion in (dict(), dict(loss_type="huber", huber_delta=0.3, loss_weighting="min_snr", prediction_type="v_prediction")):
        off = _run(name, _model(name, sd, missing_values=None, **diffusion), x=xf)
        on = _run(name, _model(name, sd, **diffusion), x=xf)
        assert on[2] & MASKED and not off[2] & MASKED
        assert on[2] & ~(MASKED | LOSS_EPI) == off[2] & ~LOSS_EPI, f"{on[2]:#x} vs {off[2]:#x}"
        bad = _compare(name, f"mask on vs off, all finite {sorted(diffusion)}", on, off)
        assert not bad, "\n".join(bad)


# ---- case 5: all-missing batch --------------------------------------------------------------------------------------------------------
def test_all_missing_batch_gives_zero_loss_and_zero_gradients():
    name = "real16"
    sd, x, cond, t, noise, injected, _ = _shape(name)
    loss, grads, path = _run(name, _model(name, sd), x=torch.full_like(x, float("nan")))
    assert loss == 0.0 and path & MASKED
    for k, g in grads.items():
        assert torch.isfinite(g).all() and bool((g == 0).all()), k


# ---- case 6: precision = "bf16x3" -----------------------------------------------------------------------------------------------------
def test_bf16x3_keeps_the_masked_loss_on_the_fp32_launcher():
    case = "full2111-l2-eps"
    name = CASES[case][0]
    got = _run(name, _case_model(case, precision="bf16x3"))
    bad = _compare(name, "bf16x3", got, _reference(case))
    assert not bad, "\n".join(bad)
    assert got[2] & MASKED and not got[2] & MSE_BF16, f"last_train_path {got[2]:#x}"
    assert got[2] & (SQ_FWD | XPAD) == SQ_FWD | XPAD


# ---- case 7: refusals on the device path ----------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_leave_the_handle_usable():
    name = "deep300"
    sd, x, cond, t, noise, injected, _ = _shape(name)
    mut, expr, pw, cd = DEEP
    m = _model(name, sd)
    xf = zero_fill(x)
    before = [p.detach().clone() for p in m.parameters()]
    m.set_constraints([[mut + 1, mut + 7, mut + 100]], list(range(4)), list(range(mut, mut + 4)), pathway_weight=0.5, mutexpr_weight=0.5)
    sentinel = [torch.full_like(p, 7.0) for p in m.parameters()]

    def refused(match):
        """The call raises naming the reason, and no gradient buffer was touched."""
        with pytest.raises(ValueError, match=match):
            _loss_fwd_bwd(m, x.cuda(), cond.cuda(), L.ptr_array(sentinel), t=t.cuda(), noise=noise.cuda(), seed=SEED)
        torch.cuda.synchronize()
        assert all(bool((g == 7.0).all()) for g in sentinel)

    refused("constraint")
    m.set_constraints()
    m.dp_max_grad_norm = 1.0
    refused("osd_set_dp_clip")
    m.dp_max_grad_norm = None
    m.eval()
    with pytest.raises(ValueError, match="per-row squared error"):
        m.row_sq_error(xf.cuda(), cond.cuda(), t.cuda(), noise=noise.cuda())
    with pytest.raises(ValueError):
        m.missing_values = "zero"
        _run(name, m, with_grads=False)
    m.train()
    for p, b in zip(m.parameters(), before):
        assert torch.equal(p, b)
    # the same handle, unmasked, on finite rows: still the fp64 oracle's loss and gradients
    m.missing_values = None
    got = _run(name, m, x=xf)
    assert not got[2] & MASKED
    ref = Fp64Oracle(sd, xf, cond, t, noise, H4, philox_masks(H4, SHAPES[name]["n"]), P_DROP).loss_and_grads("l2")
    bad = _compare(name, "unmasked call after the refusals", got, ref)
    assert not bad, "\n".join(bad)


# ---- case 8: the Trainer end to end ---------------------------------------------------------------------------------------------------
def test_trainer_trains_on_incomplete_patients(tmp_path):
    """96 synthetic patients at the deep300 dims, 40 % without the expression block, incomplete="keep", missing_values: mask, mixup 0.2,
    batch 32, one epoch through the resident path: finite losses and parameters, and the first step's flat gradient equals a direct
    _loss_fwd_bwd call on the rows, lambda and permutation that step used."""
    mut, expr, pw, cd = DEEP
    n = 96
    rng = np.random.default_rng(5)
    ids = [f"P{i:03d}" for i in range(n)]
    has_expr = np.ones(n, dtype=bool)
    has_expr[rng.permutation(n)[:38]] = False               # 38 / 96 = 40 %
    mdf = pd.DataFrame((rng.random((n, mut)) > 0.5).astype(np.float32), index=ids)
    edf = pd.DataFrame(rng.normal(size=(int(has_expr.sum()), expr)).astype(np.float32), index=[p for p, h in zip(ids, has_expr) if h])
    pdf = pd.DataFrame(rng.normal(size=(n, pw)).astype(np.float32), index=ids)
    clin = pd.DataFrame({"submitter_id": ids, "survival_days": rng.random(n) * 1000, "c0": rng.normal(size=n), "c1": rng.normal(size=n),
                         "c2": rng.normal(size=n)})
    ds = OsteosarcomaDataset(mdf, edf, pdf, clin, ["c0", "c1", "c2"], incomplete="keep")
    assert len(ds) == n and int(torch.isnan(ds.data[:, mut:mut + expr]).all(dim=1).sum()) == 38
    conf = config(H4, p=P_DROP)
    conf["training"] = {"learning_rate": LR, "weight_decay": WD, "patience": 10, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.2},
                        "save_dir": str(tmp_path), "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": 32,
                        "missing_values": "mask"}
    sd = inputs(DEEP, H4, 300)[0]
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=32, shuffle=True, num_workers=0, drop_last=True)
    tr = Trainer(m.cuda(), loader, loader, conf, device="cuda")
    steps, grads_seen, losses = [], [], []
    train_step, opt_step = tr.train_step, tr.optimizer.step

    def recording_step(*a, **k):
        steps.append(k)
        loss = train_step(*a, **k)
        losses.append(loss)
        return loss

    def recording_opt(*a, **k):
        grads_seen.append([g.detach().clone() for g in tr.flat.grad_views])
        return opt_step(*a, **k)

    tr.train_step, tr.optimizer.step = recording_step, recording_opt
    avg = tr.train_epoch()
    val = tr.validate()
    assert tr.resident and len(steps) == 3 and all(s.get("source") is not None for s in steps)
    assert np.isfinite(avg) and np.isfinite(val) and all(bool(torch.isfinite(v).all()) for v in losses)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    assert _path(m) & MASKED
    data, cond, _, idx, idx_b, lam = steps[0]["source"]
    assert idx_b is not None and bool(torch.isnan(data[idx]).any())
    fresh = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    fresh.load_state_dict(sd, strict=False)
    fresh = fresh.cuda().train()
    grads = [torch.empty_like(p) for p in fresh.parameters()]
    loss = _loss_fwd_bwd(fresh, None, None, L.ptr_array(grads), source=(data, cond, idx, idx_b, lam), seed=steps[0]["seed"])
    torch.cuda.synchronize()
    assert_close(losses[0].item(), loss.item(), LOSS_RTOL, what="first step's loss")
    for (k, _), g, ref in zip(fresh.named_parameters(), grads_seen[0], grads):
        assert_close(g.cpu(), ref.cpu(), GRAD_RTOL, atol=1e-9, what=f"first step's grad {k}")
    assert float(sum(g.abs().sum() for g in grads)) > 0
