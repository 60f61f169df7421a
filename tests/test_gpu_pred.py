"""GPU: the prediction types (config['model']['diffusion']['prediction_type'] = epsilon | v_prediction | sample) through every layer --
the target the q_sample kernels write (bits), the training step, the resident path and the constraint losses against float64
autograd, every sampler engine and the sampling options against the float64 chain unfolded at x0^ (tests/pred_helpers.py),
``predict``, the untouched default, and the checkpoint round trip.

Shapes, inputs, tolerances and path bits of the training cases are those of tests/test_gpu_loss.py (its shape groups and their fp64
forward graphs are shared, not rebuilt); model, T, S, N and the tolerance of the sampling cases are those of tests/test_gpu_ddim.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import constraints_oracle as CO
from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.ddim import ddim_timesteps
from osteosarcoma_diffusionmodel_amd.generate import load_trained_model
from osteosarcoma_diffusionmodel_amd.train import Trainer, _loss_fwd_bwd
from helpers import FULL, FULL_H, RawHandle, assert_close, config
from loss_helpers import LOSS_RTOL, P_DROP, SEED, Fp64Oracle, check, inputs
from pred_helpers import PREDICTIONS, chain64, guided_out, loss_fn, min_snr64, model_sd64, readings, row_scalars
from test_clip_cpu import mixed_bounds
from test_gpu_ddim import ATOL, ENGINES, N, RTOL, S, T, _model as ddim_model, _run as run_engine, _use
from test_gpu_known import C0_NONZERO
from test_gpu_loss import (H3, LOSS_EPI, MSE_BF16, REAL, SHAPES, SQ_FWD, XPAD, _assert_params_close, _model as loss_model, _path,
                           _run as loss_run, _shape, _step_reference, _train_conf)
from test_known_cpu import make_known

pytestmark = pytest.mark.gpu

TARGET = L.OSD_TP_TARGET
_cache = {}


# ---- the target the q_sample kernels write: bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", PREDICTIONS)
@pytest.mark.parametrize("dims,n", [((62, 5054, 26, 4), 5), ((16, 480, 16, 3), 300)])          # D = 5142: a ragged last quad; D = 512
def test_target_bits(prediction, dims, n):
    mut, expr, pw, cd = dims
    D = mut + expr + pw
    conf = config(H3)
    conf["model"]["diffusion"]["prediction_type"] = prediction
    m = BiologyAwareDiffusionModel(mut, expr, pw, cd, conf).cuda().eval()
    g = torch.Generator().manual_seed(D + n)
    x0, noise = torch.randn(n, D, generator=g), torch.randn(n, D, generator=g)
    t = torch.randint(0, 1000, (n,), generator=g)
    t[0], t[-1] = 0, 999
    sa, s1 = m.sqrt_alphas_cumprod.cpu()[t].view(-1, 1), m.sqrt_one_minus_alphas_cumprod.cpu()[t].view(-1, 1)

    def want(eps):                 # what torch forms in fp32: two rounded products, one subtraction
        return sa * eps - s1 * x0 if prediction == "v_prediction" else x0

    eps_model = BiologyAwareDiffusionModel(mut, expr, pw, cd, config(H3)).cuda().eval()
    # injected noise: the target itself, and the x_t of the plain call
    x_t, target = m.q_sample(x0.cuda(), t.cuda(), noise.cuda(), return_target=True)
    x_t_plain, _ = eps_model.q_sample(x0.cuda(), t.cuda(), noise.cuda())
    assert torch.equal(target.cpu(), want(noise)) and torch.equal(x_t, x_t_plain)
    assert target.data_ptr() != x_t.data_ptr()
    # Philox noise: the eps of the plain call at the same seed through the same expression
    x_t, target = m.q_sample(x0.cuda(), t.cuda(), seed=77, return_target=True)
    x_t_plain, eps = eps_model.q_sample(x0.cuda(), t.cuda(), seed=77)
    assert torch.equal(target.cpu(), want(eps.cpu())) and torch.equal(x_t, x_t_plain)
    # an epsilon model's target is the noise
    _, tgt = eps_model.q_sample(x0.cuda(), t.cuda(), noise.cuda(), return_target=True)
    assert torch.equal(tgt.cpu(), noise)
    _, tgt = eps_model.q_sample(x0.cuda(), t.cuda(), seed=77, return_target=True)
    assert torch.equal(tgt, eps)


# ---- the training step against fp64 autograd ---------------------------------------------------------------------------------------
SHAPE_BITS = {"real16": (0, SQ_FWD | MSE_BF16), "full2111": (SQ_FWD | XPAD, MSE_BF16), "deep300": (0, SQ_FWD | MSE_BF16)}
# case: (shape group, prediction, loss_type, huber_delta, min_snr?, precision)
TRAIN_CASES = {}
for _p in PREDICTIONS:
    for _name in ("real16", "full2111", "deep300"):
        TRAIN_CASES[f"{_name}-{_p}-l2"] = (_name, _p, "l2", 1.0, False, None)
    for _name in ("real16", "full2111"):
        TRAIN_CASES[f"{_name}-{_p}-huber-minsnr"] = (_name, _p, "huber", 1.0, True, None)
TRAIN_CASES["full2111-v_prediction-huber-b3"] = ("full2111", "v_prediction", "huber", 1.0, False, "bf16x3")


def _snr_table(prediction, gamma=5.0):
    return min_snr64(O.schedule_buffers("cosine", 1000)["alphas_cumprod"], gamma, prediction).float()


def _device(case):
    if ("dev", case) not in _cache:
        name, prediction, kind, delta, snr, precision = TRAIN_CASES[case]
        m = loss_model(name, _shape(name)[0], precision, prediction_type=prediction, loss_type=kind, huber_delta=delta,
                       loss_weighting="min_snr" if snr else None)
        _cache[("dev", case)] = loss_run(name, m)
    return _cache[("dev", case)]


def _reference(name, prediction, kind="l2", delta=1.0, weights=None, flip_b=False):
    key = ("ref", name, prediction, kind, delta, None if weights is None else float(weights.double().sum()), flip_b)
    if key not in _cache:
        orc = _shape(name)[6]
        _cache[key] = orc.grads_of(loss_fn(orc, prediction, kind, delta, weights, flip_b))
    return _cache[key]


def _compare(name, tag, got, ref):
    loss, grads, _ = got
    worst, bad = check(loss, grads, ref[0], ref[1], sum(SHAPES[name]["dims"][:3]))
    print(f"[{name} {tag}] loss {loss:.8g} (fp64 {ref[0]:.8g}); worst error / tolerance {worst:.3f}")
    return bad


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_vs_fp64_autograd(case):
    name, prediction, kind, delta, snr, precision = TRAIN_CASES[case]
    got = _device(case)
    ref = _reference(name, prediction, kind, delta, _snr_table(prediction) if snr else None)
    bad = _compare(name, case, got, ref)
    assert not bad, "\n".join(bad)
    path = got[2]
    want_set, want_clear = SHAPE_BITS[name]
    if precision == "bf16x3":
        want_set, want_clear = want_set | MSE_BF16, want_clear & ~MSE_BF16
    assert path & TARGET, f"last_train_path {path:#x}: OSD_TP_TARGET is not set"
    assert bool(path & LOSS_EPI) == (kind != "l2" or snr), f"last_train_path {path:#x}"
    assert path & want_set == want_set and not path & want_clear, f"last_train_path {path:#x}, wanted {want_set:#x} set and {want_clear:#x} clear"


@pytest.mark.parametrize("prediction", PREDICTIONS)
def test_l1_loss_value(prediction):
    """l1 on the loss value only: its gradient jumps at the kink and the shape groups' noise is conditioned around the eps target."""
    name = "real16"
    m = loss_model(name, _shape(name)[0], prediction_type=prediction, loss_type="l1")
    loss, _, path = loss_run(name, m, with_grads=False)
    orc = _shape(name)[6]
    ref = loss_fn(orc, prediction, "l1")(orc.pred.detach()).item()
    print(f"[{name} {prediction} l1] loss {loss:.8g} (fp64 {ref:.8g})")
    assert_close(loss, ref, LOSS_RTOL, what="l1 loss")
    assert path & TARGET and path & LOSS_EPI


def test_negative_controls_training():
    """The tolerance separates: each wrong oracle lies outside it in the loss or in at least one gradient tensor."""
    v_l2, x0_l2 = _device("real16-v_prediction-l2"), _device("real16-sample-l2")
    assert _compare("real16", "v against the eps target", v_l2, _reference("real16", "epsilon")), "an eps target went unnoticed"
    assert _compare("real16", "v against b flipped", v_l2, _reference("real16", "v_prediction", flip_b=True)), "a flipped b went unnoticed"
    assert _compare("real16", "sample against the v target", x0_l2, _reference("real16", "v_prediction")), "the wrong target went unnoticed"
    v_snr = _device("real16-v_prediction-huber-minsnr")
    wrong = _reference("real16", "v_prediction", "huber", 1.0, _snr_table("epsilon"))
    assert _compare("real16", "v + min_snr against the eps form of the weights", v_snr, wrong), "the eps form of min-SNR went unnoticed"
    orc = _shape("real16")[6]
    le, lv = (loss_fn(orc, p)(orc.pred.detach()).item() for p in ("epsilon", "v_prediction"))
    print(f"[real16] fp64 l2: eps {le:.8g}, v {lv:.8g}, relative distance {abs(le - lv) / le:.2e} ({abs(le - lv) / le / LOSS_RTOL:.1f} x the loss tolerance)")
    assert abs(le - lv) > LOSS_RTOL * le


def test_default_path_has_no_target_bit():
    got = loss_run("real16", loss_model("real16", _shape("real16")[0]), with_grads=False)
    assert not got[2] & TARGET and not got[2] & LOSS_EPI


# ---- the resident path: gather + mixup + q_sample + target in one pass ----------------------------------------------------------------
def test_trainer_resident_step_with_mixup_and_validate(tmp_path, monkeypatch):
    """One Trainer.train_step on rows of a device-resident dataset with mixup on and prediction_type: v_prediction against
    O.clip_grad_norm + O.adamw_step on the fp64 gradients of the mixed batch (x0 of the target is the mixed row); Trainer.validate
    returns the v loss."""
    from osteosarcoma_diffusionmodel_amd import train as TR
    from osteosarcoma_diffusionmodel_amd.train import OsteosarcomaDataset
    sd, x, cond, t, noise, injected, _ = _shape("real16")
    n, lam = x.shape[0], 0.3
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    xm = lam * x + (1.0 - lam) * x[perm]               # MixupAugmentation in fp32: two rounded products, one addition
    cm = lam * cond + (1.0 - lam) * cond[perm]
    orc = Fp64Oracle(sd, xm, cm, t, noise, H3, injected, P_DROP)
    ref_loss, ref_grads = orc.grads_of(loss_fn(orc, "v_prediction"))
    plain = _shape("real16")[6]
    unmixed = loss_fn(plain, "v_prediction")(plain.pred.detach()).item()
    conf = _train_conf(H3, tmp_path, prediction_type="v_prediction")
    mut, expr, pw, cd = REAL
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    ds = object.__new__(OsteosarcomaDataset)
    ds.data, ds.conditions, ds.survival_days = x.clone(), cond.clone(), torch.rand(n) * 1000
    loader = torch.utils.data.DataLoader(ds, batch_size=n, shuffle=False, num_workers=0)
    tr = Trainer(m, loader, loader, conf, device="cuda")
    # validate: eval mode, resident rows, t / noise injected into its call
    ev = _shape("real16-eval")
    val_ref = loss_fn(ev[6], "v_prediction")(ev[6].pred.detach()).item()
    eps_ref = loss_fn(ev[6], "epsilon")(ev[6].pred.detach()).item()
    orig, calls = TR._loss_fwd_bwd, []

    def injected_draws(*a, **k):
        calls.append(k.get("source") is not None)
        return orig(*a, t=t.cuda(), noise=ev[4].cuda(), **k)

    monkeypatch.setattr(TR, "_loss_fwd_bwd", injected_draws)
    val = tr.validate()
    monkeypatch.setattr(TR, "_loss_fwd_bwd", orig)
    print(f"[resident] validate {val:.8g} (fp64 v {val_ref:.8g}, fp64 eps {eps_ref:.8g})")
    assert calls == [True] and tr.resident
    assert_close(val, val_ref, LOSS_RTOL, what="validate")
    assert abs(val_ref - eps_ref) > LOSS_RTOL * val_ref
    m.train()
    idx = torch.arange(n, device="cuda")
    source = (x.cuda(), cond.cuda(), None, idx, idx[perm.cuda()], lam)
    loss = tr.train_step(None, None, source=source, t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in injected])
    path = _path(m)
    print(f"[resident] train_step loss {loss.item():.8g} (fp64 mixed {ref_loss:.8g}, unmixed {unmixed:.8g})")
    assert_close(loss.item(), ref_loss, LOSS_RTOL, what="train_step loss")
    assert abs(ref_loss - unmixed) > LOSS_RTOL * ref_loss
    assert path & TARGET and not path & LOSS_EPI
    names, clipped, norm, p1 = _step_reference(ref_grads, sd)
    assert_close(tr.optimizer.grad_norm.item(), norm.item(), 2e-5, what="pre-clip gradient norm")
    for k, p in m.named_parameters():
        j = names.index(k)
        _assert_params_close(p.detach().cpu(), p1[j], clipped[j], k)


def test_trainer_follows_a_type_changed_after_construction(tmp_path):
    """The Trainer's fast path keeps its engine: model.prediction_type assigned after construction reaches the next step (target and
    min-SNR form alike), and an unknown value raises there."""
    sd, x, cond, t, noise, injected, orc = _shape("real16")
    conf = _train_conf(H3, tmp_path, loss_weighting="min_snr")
    mut, expr, pw, cd = REAL
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()
    tr = Trainer(m, [], [], conf, device="cuda")
    m.prediction_type = "v_prediction"
    ref_loss, ref_grads = _reference("real16", "v_prediction", "l2", 1.0, _snr_table("v_prediction"))
    kw = dict(t=t.cuda(), noise=noise.cuda(), dropout_masks=[k.cuda() for k in injected])
    loss = tr.train_step(x.cuda(), cond.cuda(), **kw)
    path = _path(m)
    assert_close(loss.item(), ref_loss, LOSS_RTOL, what="train_step loss")
    assert path & TARGET and path & LOSS_EPI
    names, clipped, norm, p1 = _step_reference(ref_grads, sd)
    assert_close(tr.optimizer.grad_norm.item(), norm.item(), 2e-5, what="pre-clip gradient norm")
    for k, p in m.named_parameters():
        j = names.index(k)
        _assert_params_close(p.detach().cpu(), p1[j], clipped[j], k)
    m.prediction_type = "velocity"
    with pytest.raises(ValueError):
        tr.train_step(x.cuda(), cond.cuda(), **kw)


# ---- the constraint losses read x0^ = a x_t - b out ---------------------------------------------------------------------------------------
def test_constraints_with_v_vs_fp64_autograd():
    """set_constraints + v_prediction at dims (16, 224, 16, 3), 256 rows, eval mode, against fp64 autograd of the composite, at the
    tolerances of tests/test_gpu_constraints.py (totals and parts 2e-5, gradients 1e-4 * max|ref| + 1e-9)."""
    dims, hidden, n = (16, 224, 16, 3), H3, 256
    sd, x0, cond, t, noise, _ = inputs(dims, hidden, n)
    mut, expr, pwd, cd = dims
    D = mut + expr + pwd
    pw = [[mut + 1, mut + 7, mut + 100, mut + 201], [mut + 3, mut + expr - 1, D - 2], [mut + 5, mut + 6, mut + 9, D - 1]]
    ca, cb = list(range(0, 16)), list(range(mut + expr - 16, mut + expr))
    w_pc, w_me = 0.7, 1.3
    orc = Fp64Oracle(sd, x0, cond, t, noise, hidden)
    a, b = row_scalars(orc.bufs, t)
    v_loss = loss_fn(orc, "v_prediction")
    parts = {}

    def composite(pred, reading="v_prediction"):
        main = v_loss(pred)
        x_t = O.q_sample(orc.bufs, x0.double(), t, noise.double())
        xh = readings(reading, a, b, x_t, pred)["x0"]
        l_pc = CO.pathway_coherence_loss(xh, pw)
        l_me = CO.mutation_expression_correlation_loss(xh, x0.double(), ca, cb)
        parts.update(main=main.item(), pc=l_pc.item(), me=l_me.item())
        return main + w_pc * l_pc + w_me * l_me

    wrong_total = composite(orc.pred.detach(), "epsilon").item()        # x0^ read as an eps model would
    total, ref = orc.grads_of(composite)
    conf = config(hidden, p=P_DROP)
    conf["model"]["diffusion"]["prediction_type"] = "v_prediction"
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pwd, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.set_constraints(pw, ca, cb, pathway_weight=w_pc, mutexpr_weight=w_me)
    loss = m(x0.cuda(), cond.cuda(), t=t.cuda(), noise=noise.cuda())
    loss.backward()
    path = _path(m)
    got = m.last_loss_parts()
    print(f"[cons] total {loss.item():.8g} (fp64 {total:.8g}; with the eps reading of x0^ {wrong_total:.8g}); parts {got} (fp64 {parts})")
    assert_close(loss.item(), total, 2e-5, what="total loss")
    assert_close(got[0], parts["main"], 2e-5, what="v part")
    assert_close(got[1], parts["pc"], 2e-5, atol=1e-7, what="L_pc part")
    assert_close(got[2], parts["me"], 2e-5, atol=1e-7, what="L_me part")
    assert abs(wrong_total - total) > 2e-5 * abs(total)
    named = dict(m.named_parameters())
    for k, gr in ref.items():
        assert_close(named[k].grad.cpu(), gr, 1e-4, atol=1e-9, what=f"grad {k}")
    assert path & TARGET and not path & LOSS_EPI


# ---- sampling against the fp64 chain, unfolded at x0^ --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    m = ddim_model()
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(N, 3, generator=g)
    x_T = torch.randn(N, m.data_dim, generator=g)
    zs = torch.randn(S - 1, N, m.data_dim, generator=g)
    zs_ddpm = torch.randn(T - 1, N, m.data_dim, generator=g)
    c = dict(cond=cond, x_T=x_T, zs=zs, zs_ddpm=zs_ddpm, taus=ddim_timesteps(T, S), sd64=model_sd64(m), refs={},
             dev=dict(cond=cond.cuda(), x_T=x_T.cuda(), zs=zs.cuda(), zs_ddpm=zs_ddpm.cuda()))
    yield m, c
    m.prediction_type = "epsilon"


def _ref(case_, prediction, eta, read_as=None, taus="plan"):
    """The fp64 chain of the case: eta None = the DDPM chain.  read_as: the reading the oracle gives a model of type ``prediction``."""
    m, c = case_
    key = (prediction, eta, read_as, taus if isinstance(taus, str) else "shifted")
    if key not in c["refs"]:
        if eta is None:
            c["refs"][key] = chain64(m, c["cond"], c["x_T"], lambda s: c["zs_ddpm"][T - 1 - s], None, 1.0, read_as or prediction, sd=c["sd64"])
        else:
            tt = c["taus"] if isinstance(taus, str) else taus
            c["refs"][key] = chain64(m, c["cond"], c["x_T"], lambda s: c["zs"][S - 1 - s], tt, eta, read_as or prediction, sd=c["sd64"])
    return c["refs"][key]


def _sample(case_, engine, prediction, eta):
    m, c = case_
    m.prediction_type = prediction
    d = c["dev"]
    if eta is None:
        return run_engine(m, engine, d["cond"], N, x_T=d["x_T"], noise=d["zs_ddpm"], seed=3)
    return run_engine(m, engine, d["cond"], N, x_T=d["x_T"], noise=d["zs"] if eta > 0 else None, seed=3, num_inference_steps=S, eta=eta)


@pytest.mark.parametrize("eta", [0.0, 0.5, None], ids=["eta0", "eta0.5", "ddpm"])
@pytest.mark.parametrize("prediction", PREDICTIONS)
@pytest.mark.parametrize("engine", list(ENGINES))
def test_sampling_vs_fp64_chain(case, engine, prediction, eta):
    m = case[0]
    out, mask = _sample(case, engine, prediction, eta)
    ref = _ref(case, prediction, eta)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"{engine} {prediction} eta={eta}: max|ref|={ref.abs().max().item():.3e} err={err:.3e} tol={ATOL + RTOL * ref.abs().max().item():.3e}")
    assert_close(out, ref, RTOL, ATOL, f"{engine} {prediction} eta={eta}")
    assert torch.equal(mask, (out[:, :m.mutation_dim] > 0.5).float())


@pytest.mark.parametrize("prediction", PREDICTIONS)
def test_sampling_bf16x3(case, prediction):
    m = case[0]
    m.precision = "bf16x3"
    try:
        out, _ = _sample(case, "layers_graph", prediction, 0.5)
        assert m.last_precision == "bf16x3"
    finally:
        m.precision = None
    assert_close(out, _ref(case, prediction, 0.5), RTOL, ATOL, f"bf16x3 {prediction}")


def test_negative_controls_sampling(case):
    """The tolerance separates: a v model's chain against the oracle that reads its output as eps, and against timesteps moved by one."""
    m, c = case
    out, _ = _sample(case, "layers_graph", "v_prediction", 0.5)
    ref = _ref(case, "v_prediction", 0.5)
    assert_close(out, ref, RTOL, ATOL, "control")
    tol = ATOL + RTOL * ref.abs().max().item()
    as_eps = _ref(case, "v_prediction", 0.5, read_as="epsilon")
    shifted = _ref(case, "v_prediction", 0.5, taus=c["taus"] - 1)
    print(f"max|x| of the chain: v reading {ref.abs().max().item():.3g}, eps reading of the same outputs {as_eps.abs().max().item():.3g}")
    assert (out.cpu().double() - as_eps).abs().max().item() > tol
    assert (out.cpu().double() - shifted).abs().max().item() > tol
    out_d, _ = _sample(case, "layers_graph", "v_prediction", None)
    assert (out_d.cpu().double() - _ref(case, "v_prediction", None, read_as="epsilon")).abs().max().item() > tol


@pytest.mark.parametrize("prediction", PREDICTIONS)
def test_engines_among_themselves(case, prediction):
    """Philox draws: the per-layer engines and the workspace / panel chain kernels agree bit for bit, the squad kernels to fp32 rounding
    and with themselves (as tests/test_gpu_ddim.py asserts for the eps model); strided and DDPM."""
    m, c = case
    m.prediction_type = prediction
    cond = c["dev"]["cond"]
    for kw in (dict(seed=77, row_offset=5, num_inference_steps=S, eta=0.5), dict(seed=78, row_offset=5)):
        ref, ref_mask = run_engine(m, "layers_graph", cond, N, **kw)
        assert bool(torch.isfinite(ref).all())
        for engine in ("layers_eager", "workspace", "panel"):
            out, mask = run_engine(m, engine, cond, N, **kw)
            assert torch.equal(out, ref) and torch.equal(mask, ref_mask), (engine, kw)
        for engine in ("squad32", "squad16"):
            out, _ = run_engine(m, engine, cond, N, **kw)
            assert_close(out, ref, 2e-5, 1e-6, engine)
            again, _ = run_engine(m, engine, cond, N, **kw)
            assert torch.equal(again, out), f"{engine} against itself"


# ---- the sampling options: guidance + known + x0 bounds in one chain (per-layer kernels) ------------------------------------------------------
@pytest.mark.parametrize("mode", ["ddim", "ddpm"])
@pytest.mark.parametrize("prediction", PREDICTIONS)
def test_options_vs_fp64_restatement(case, prediction, mode):
    m, c = case
    m.prediction_type = prediction
    _use(m, "layers_graph")
    lo, hi = mixed_bounds()
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(N, m.data_dim, generator=g)
    x0[:, :m.mutation_dim] = (x0[:, :m.mutation_dim] > 0).float()
    kn = make_known(x0, "thirty_percent", seed=31)
    obs = ~torch.isnan(kn)
    kn = torch.where(obs, torch.minimum(torch.maximum(kn, torch.from_numpy(lo)), torch.from_numpy(hi)), kn)
    guide = guided_out(3.0, C0_NONZERO)
    if mode == "ddim":
        zs, kw = c["zs"], dict(num_inference_steps=S, eta=0.5)
        ref = chain64(m, c["cond"], c["x_T"], lambda s: zs[S - 1 - s], c["taus"], 0.5, prediction, sd=c["sd64"], out_fn=guide, known=kn, lo=lo, hi=hi)
        zs_dev = c["dev"]["zs"]
    else:
        zs, kw = c["zs_ddpm"], {}
        ref = chain64(m, c["cond"], c["x_T"], lambda s: zs[T - 1 - s], None, 1.0, prediction, sd=c["sd64"], out_fn=guide, known=kn, lo=lo, hi=hi)
        zs_dev = c["dev"]["zs_ddpm"]
    m.null_condition = C0_NONZERO
    try:
        out, mask = m.sample(c["dev"]["cond"], N, x_T=c["dev"]["x_T"], noise=zs_dev, known=kn.cuda(), x0_bounds=(lo, hi), guidance_scale=3.0,
                             return_mutation_mask=True, **kw)
    finally:
        m.null_condition = None
    assert m.last_sampler == "graph"
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"options {prediction} {mode}: max|ref|={ref.abs().max().item():.3e} err={err:.3e} tol={ATOL + RTOL * ref.abs().max().item():.3e}")
    assert_close(out, ref, RTOL, ATOL, f"options {prediction} {mode}")
    obs_d = obs.cuda()
    assert torch.equal(out[obs_d], kn.cuda()[obs_d])                       # observed elements come back bit for bit
    lo_t, hi_t = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    assert bool((((out >= lo_t) & (out <= hi_t)) | obs_d).all())          # every free element inside its bounds
    assert bool(obs.any()) and bool((~obs).any())
    assert torch.equal(mask, (out[:, :m.mutation_dim] > 0.5).float())


@pytest.mark.parametrize("prediction", ("epsilon",) + PREDICTIONS)
def test_guidance_on_the_raw_output_is_guidance_in_eps_space(case, prediction):
    """fp64: out(c0) + w (out(c) - out(c0)) read as eps equals eps(c0) + w (eps(c) - eps(c0)), for every type, to 1e-12 of max|eps|."""
    m, c = case
    sd, w = c["sd64"], 3.0
    n = 32
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, m.data_dim, generator=g, dtype=torch.float64)
    cond = c["cond"][:n].double()
    c0 = torch.tensor(C0_NONZERO, dtype=torch.float64).reshape(1, -1).repeat(n, 1)
    for tau in (0, 37, T - 1):
        a = m.sqrt_alphas_cumprod.cpu().double()[tau]
        b = m.sqrt_one_minus_alphas_cumprod.cpu().double()[tau]
        t_norm = torch.full((n,), tau / T, dtype=torch.float64)
        out_c = O.unet_forward(sd, x, t_norm, O.condition_embed(sd, cond), len(FULL_H), 128, None, 0.0)
        out_u = O.unet_forward(sd, x, t_norm, O.condition_embed(sd, c0), len(FULL_H), 128, None, 0.0)
        raw = readings(prediction, a, b, x, out_u + w * (out_c - out_u))["eps"]
        e_c, e_u = readings(prediction, a, b, x, out_c)["eps"], readings(prediction, a, b, x, out_u)["eps"]
        in_eps = e_u + w * (e_c - e_u)
        assert (raw - in_eps).abs().max().item() <= 1e-12 * in_eps.abs().max().item(), (prediction, tau)
        assert (e_c - e_u).abs().max().item() > 1e-6 * in_eps.abs().max().item()          # the two branches differ


# ---- predict -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", PREDICTIONS)
def test_predict_readings(case, prediction):
    """(300, 2000): as_ = x0 | eps | v of a v model and of a sample model against the fp64 conversions at the forward tolerance of
    tests/test_gpu_model.py (1e-5 * max|ref|); the three satisfy x_t = a x0^ + b eps^ to that tolerance."""
    m, c = case
    m.prediction_type = prediction
    _use(m, "layers_graph")
    g = torch.Generator().manual_seed(21)
    x_t = torch.randn(N, m.data_dim, generator=g)
    t = torch.randint(0, T, (N,), generator=g)
    t[0], t[1] = 0, T - 1
    sd = c["sd64"]
    out64 = O.unet_forward(sd, x_t.double(), t.double() / T, O.condition_embed(sd, c["cond"].double()), len(FULL_H), 128, None, 0.0)
    a = m.sqrt_alphas_cumprod.cpu().double()[t].view(-1, 1)
    b = m.sqrt_one_minus_alphas_cumprod.cpu().double()[t].view(-1, 1)
    want = readings(prediction, a, b, x_t.double(), out64)
    got = {}
    with torch.no_grad():
        raw = m.predict(x_t.cuda(), t.cuda(), c["dev"]["cond"])
        assert_close(raw, out64, 1e-5, what="raw")
        for as_ in ("x0", "eps", "v"):
            got[as_] = m.predict(x_t.cuda(), t.cuda(), c["dev"]["cond"], as_=as_)
            assert_close(got[as_], want[as_], 1e-5, what=f"{prediction} as {as_}")
        assert torch.equal(got["v" if prediction == "v_prediction" else "x0"], raw)          # the model's own reading is the output
        assert torch.equal(m.predict_noise(x_t.cuda(), t.cuda(), c["dev"]["cond"]), got["eps"])     # a real eps^
        back = a * got["x0"].cpu().double() + b * got["eps"].cpu().double()
        assert_close(back, x_t.double(), 1e-5, what="a x0^ + b eps^ against x_t")
        one = m.predict(x_t.cuda(), 37, c["dev"]["cond"], as_="x0")                            # a shared python-int t
        rows = m.predict(x_t.cuda(), torch.full((N,), 37).cuda(), c["dev"]["cond"], as_="x0")
        assert torch.equal(one, rows)
        with pytest.raises(ValueError):
            m.predict(x_t.cuda(), t.cuda(), c["dev"]["cond"], as_="noise")


# ---- nothing moves by default -----------------------------------------------------------------------------------------------------------------
def _small_training_call(prediction=None, switch_from=None):
    """tests/test_gpu_loss.py's reproducible shape: (loss, gradients, path) of one training call."""
    dims, hidden, n = (8, 24, 8, 3), [32, 64, 32], 16
    sd, x, cond, t, noise, injected = inputs(dims, hidden, n)
    mut, expr, pw, cd = dims
    conf = config(hidden, p=P_DROP)
    if prediction is not None:
        conf["model"]["diffusion"]["prediction_type"] = prediction
    m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().train()

    def call():
        grads = [torch.empty_like(p) for p in m.parameters()]
        loss = _loss_fwd_bwd(m, x.cuda(), cond.cuda(), L.ptr_array(grads), t=t.cuda(), noise=noise.cuda(), seed=SEED,
                             dropout_masks=[k.cuda() for k in injected])
        torch.cuda.synchronize()
        return loss.cpu(), [g.cpu() for g in grads], _path(m)

    if switch_from is not None:
        m.prediction_type = switch_from
        other = call()
        assert other[2] & TARGET
        m.prediction_type = prediction or "epsilon"
        return call(), other
    return call()


def test_default_is_unchanged():
    """A config without the key and one that says "epsilon": equal bits for a training call and for sample on the per-layer and squad
    engines, OSD_TP_TARGET absent; a live model switched v -> epsilon has the bits of a fresh epsilon model."""
    base, again, named = _small_training_call(), _small_training_call(), _small_training_call("epsilon")
    assert torch.equal(base[0], again[0]) and all(torch.equal(p, q) for p, q in zip(base[1], again[1])), "the default step is not reproducible here"
    assert torch.equal(base[0], named[0]) and all(torch.equal(p, q) for p, q in zip(base[1], named[1]))
    assert not base[2] & TARGET and base[2] == named[2]
    switched, as_v = _small_training_call(None, switch_from="v_prediction")
    assert torch.equal(base[0], switched[0]) and all(torch.equal(p, q) for p, q in zip(base[1], switched[1])) and switched[2] == base[2]
    assert not torch.equal(as_v[0], base[0])
    # sampling: three models with the same parameters
    plain = ddim_model(seed=2)
    conf = config(FULL_H, T=T)
    conf["model"]["diffusion"]["prediction_type"] = "epsilon"
    named_m = BiologyAwareDiffusionModel(config=conf, **FULL).cuda().eval()
    named_m.load_state_dict(plain.state_dict())
    named_m.input_splitk = 0
    live = ddim_model(seed=2)
    cond = torch.randn(N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    for engine in ("layers_graph", "squad32"):
        for kw in (dict(seed=77, row_offset=5, num_inference_steps=S, eta=0.5), dict(seed=78)):
            ref, ref_mask = run_engine(plain, engine, cond, N, **kw)
            out, mask = run_engine(named_m, engine, cond, N, **kw)
            assert torch.equal(out, ref) and torch.equal(mask, ref_mask), (engine, kw)
            live.prediction_type = "v_prediction"
            as_v, _ = run_engine(live, engine, cond, N, **kw)
            live.prediction_type = "epsilon"
            out, mask = run_engine(live, engine, cond, N, **kw)
            assert torch.equal(out, ref) and torch.equal(mask, ref_mask), (engine, kw, "v -> epsilon")
            assert not torch.equal(as_v, ref)
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(live._engine().handle, b"prediction_type", C.byref(v)))
    assert v.value == L.OSD_PRED_EPSILON
    live.prediction_type = "sample"
    L.check(L.lib().osd_get_option(live._engine().handle, b"prediction_type", C.byref(v)))
    assert v.value == L.OSD_PRED_SAMPLE
    live.prediction_type = "velocity"
    with pytest.raises(ValueError):
        live.sample(cond, N, num_inference_steps=S)


# ---- round trip and errors ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    import pandas as pd
    conf = _train_conf(FULL_H, tmp_path, prediction_type="v_prediction", num_steps=T)
    conf["training"]["ema_decay"] = 0.999
    torch.manual_seed(3)
    m = BiologyAwareDiffusionModel(config=conf, **FULL).cuda()
    tr = Trainer(m, [], [], conf, device="cuda")
    tr.save_checkpoint(0, 0.0)
    for fname, width in (("mutation_matrix_aligned.csv", FULL["mutation_dim"]), ("expression_matrix_aligned.csv", FULL["expression_dim"]),
                         ("pathway_scores.csv", FULL["pathway_dim"])):
        pd.DataFrame(np.zeros((1, width)), index=["p0"]).to_csv(tmp_path / fname)
    load_conf = config(FULL_H, T=T)
    assert "prediction_type" not in load_conf["model"]["diffusion"]
    load_conf["data"] = {"processed_dir": str(tmp_path)}
    cond = torch.randn(64, 3, generator=torch.Generator().manual_seed(1)).cuda()
    m.eval()
    want = m.sample(cond, 64, seed=5, num_inference_steps=S)
    eps_reading = None
    for use_ema in (None, False, True):         # no update yet: the average is the parameters
        got = load_trained_model(tmp_path / "checkpoint_epoch_0.pt", load_conf, "cuda", use_ema=use_ema)
        assert got.prediction_type == "v_prediction"
        assert torch.equal(got.sample(cond, 64, seed=5, num_inference_steps=S), want), use_ema
        got.prediction_type = "epsilon"
        eps_reading = got.sample(cond, 64, seed=5, num_inference_steps=S)
    assert not torch.equal(eps_reading, want)
    load_conf["model"]["diffusion"]["prediction_type"] = "epsilon"
    with pytest.raises(ValueError, match="prediction_type"):
        load_trained_model(tmp_path / "checkpoint_epoch_0.pt", load_conf, "cuda")


def test_osd_set_prediction_errors():
    rh = RawHandle()
    try:
        lib = L.lib()
        for bad in (3, -1, 99):
            assert lib.osd_set_prediction(rh.h, bad) == L.OSD_EINVAL and L.last_error()
        assert lib.osd_set_prediction(rh.h, L.OSD_PRED_V) == L.OSD_ESTATE and "osd_set_schedule" in L.last_error()
        assert lib.osd_set_prediction(None, L.OSD_PRED_V) == L.OSD_EINVAL
        v = C.c_int64(-1)
        L.check(lib.osd_get_option(rh.h, b"prediction_type", C.byref(v)))
        assert v.value == L.OSD_PRED_EPSILON
    finally:
        rh.close()
