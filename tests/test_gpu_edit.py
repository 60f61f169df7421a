"""GPU: counterfactual patients -- the noise map (osd_noise_map: k_q_sample_map, EpiNoiseMap) against its
definition in float64, its invariances (generated draws, launch groups, shards, repeats), the round trip through the chain, DDIM
inversion, model.edit, SyntheticPatientGenerator.counterfactual, the refusals and BiologicalValidator.counterfactual_consistency."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator, _lib as L
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table, edit_timesteps
from osteosarcoma_diffusionmodel_amd.transform import FeatureTransform
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator
from edit_helpers import ddim_inversion_oracle, noise_map_definition, oracle_denoiser, replay
from helpers import FULL, FULL_H, TAG_QNOISE, RawHandle, assert_close, config, philox_normals

pytestmark = pytest.mark.gpu

T, PLAN, N = 100, 10, 300                  # N = 300: two full 128-row tiles and a 44-row tail
STRENGTH, ETA = 0.9, 1.0
LEVELS = edit_timesteps(T, PLAN, STRENGTH)   # [0, 9, 19, ..., 89]: S = 10 levels
S = int(LEVELS.size)
RTOL, ATOL = 5e-5, 1e-5                    # test_gpu_ddim.py's: 5e-5 * max|ref| + 1e-5
KW = dict(num_inference_steps=PLAN, strength=STRENGTH, eta=ETA)


def _model(prediction="epsilon", seed=0, T_=T, **dims):
    torch.manual_seed(seed)
    d = dict(FULL)
    d.update(dims)
    conf = config(FULL_H, T=T_)
    conf["model"]["diffusion"]["prediction_type"] = prediction
    m = BiologyAwareDiffusionModel(config=conf, **d).cuda().eval()
    m.input_splitk = 0
    m.sampler, m.use_graph = "graph", True
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                  # non-trivial GroupNorm affine, as test_gpu_ddim.py
        for k, prm in m.named_parameters():
            if k.endswith((".1.weight", ".5.weight")):
                prm.copy_((1 + 0.2 * torch.randn(prm.shape, generator=gen)).cuda())
            if k.endswith((".1.bias", ".5.bias")):
                prm.copy_((0.1 * torch.randn(prm.shape, generator=gen)).cuda())
    return m


def _sd(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items() if k.startswith(("condition_embed", "unet"))}


def _plan(m, levels=LEVELS, eta=ETA):
    return ddim_step_table(m.alphas_cumprod, levels, eta, m.prediction_type, sqrt_alphas_cumprod=m.sqrt_alphas_cumprod,
                           sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod)


def _definition(m, x0, cond, eps, taus, coef):
    """(y, cz, outs) of the noise map in float64 over the oracle's denoiser: the fp32 buffers and table rows, widened."""
    a, b = m.sqrt_alphas_cumprod.detach().cpu().double(), m.sqrt_one_minus_alphas_cumprod.detach().cpu().double()
    den = oracle_denoiser(O, _sd(m), cond, taus, m.num_steps, len(FULL_H))
    return noise_map_definition(x0.double(), eps.double(), a, b, taus, torch.from_numpy(coef.astype(np.float64)), den)


def _cz(rec_noise, coef):
    """C_s z_s of a device result, in the chain's draw order: what the chain adds."""
    n_s = coef.shape[0]
    c = torch.tensor([float(coef[n_s - 1 - k, 2]) for k in range(n_s - 1)], dtype=torch.float64)
    return rec_noise.detach().cpu().double() * c[:, None, None]


def _inputs(D, n=N, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g), torch.randn(n, D, generator=g), torch.randn(S, n, D, generator=g)


_cases = {}


def _case(prediction, **dims):
    """One model, its inputs, the float64 definition and the device's injected-noise inversion, shared by the tests."""
    key = (prediction, tuple(sorted(dims.items())))
    if key not in _cases:
        m = _model(prediction, **dims)
        cond, x0, eps = _inputs(m.data_dim)
        taus, coef = _plan(m)
        y, cz, outs = _definition(m, x0, cond, eps, taus, coef)
        rec = m.invert(x0.cuda(), cond.cuda(), method="ddpm", noise=eps.cuda(), **KW)
        torch.cuda.synchronize()
        _cases[key] = dict(m=m, cond=cond, x0=x0, eps=eps, taus=taus, coef=coef, y=y, cz=torch.stack(cz), outs=outs, rec=rec)
    return _cases[key]


def _assert_map(rec, c, what):
    assert np.array_equal(rec.timesteps, LEVELS) and rec.method == "ddpm" and rec.eta == ETA
    assert tuple(rec.noise.shape) == (S - 1, c["x0"].shape[0], c["x0"].shape[1])
    assert_close(rec.x_start, c["y"][-1], RTOL, ATOL, what + ": x_start")
    assert_close(_cz(rec.noise, c["coef"]), c["cz"], RTOL, ATOL, what + ": C z")


# ---- 4. against the definition in float64, injected draws --------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["epsilon", "v_prediction", "sample"])
def test_noise_map_against_fp64(prediction):
    c = _case(prediction)
    _assert_map(c["rec"], c, prediction)


def test_noise_map_d_not_multiple_of_4():
    """expression_dim = 1901: D = 2001, the guarded operand paths of both kernels."""
    c = _case("epsilon", expression_dim=1901)
    assert c["m"].data_dim % 4 == 1
    _assert_map(c["rec"], c, "D = 2001")


def test_noise_map_negative_control():
    """The tolerance separates: the definition with the timesteps moved down by one lies outside it."""
    c = _case("epsilon")
    m = c["m"]
    moved = np.maximum(LEVELS - 1, 0).astype(np.int32)
    taus, coef = _plan(m, moved)
    y, cz, _ = _definition(m, c["x0"], c["cond"], c["eps"], taus, coef)
    cz = torch.stack(cz)
    got = _cz(c["rec"].noise, c["coef"])
    assert (got - cz).abs().max().item() > ATOL + RTOL * cz.abs().max().item()
    assert (c["rec"].x_start.cpu().double() - y[-1]).abs().max().item() > ATOL + RTOL * y[-1].abs().max().item()


def test_single_level_plan():
    """A plan of one level (strength so small that only timestep 0 is left) solves nothing: x_start = y_0, no draws, and edit returns the
    model's x0^ there."""
    c = _case("epsilon")
    m = c["m"]
    xd, cd = c["x0"].cuda(), c["cond"].cuda()
    rec = m.invert(xd, cd, method="ddpm", num_inference_steps=T, strength=0.01, noise=c["eps"][:1].cuda())
    assert rec.timesteps.tolist() == [0] and tuple(rec.noise.shape) == (0, N, m.data_dim)
    assert_close(rec.x_start, c["y"][0], RTOL, ATOL, "x_start of a one-level plan")
    got = m.edit(xd, cd, cd, method="ddpm", num_inference_steps=T, strength=0.01, noise=c["eps"][:1].cuda())
    assert_close(got, float(c["coef"][0, 0]) * c["y"][0] + float(c["coef"][0, 1]) * c["outs"][0], RTOL, ATOL, "edit over a one-level plan")


# ---- 5. generated draws ----------------------------------------------------------------------------------------------------
def test_generated_draws_are_the_documented_philox_blocks():
    c = _case("epsilon")
    m, seed, roff = c["m"], 77, 5
    eps = torch.from_numpy(np.stack([philox_normals(seed, N, m.data_dim, int(t), TAG_QNOISE, roff) for t in LEVELS]).astype(np.float32))
    gen = m.invert(c["x0"].cuda(), c["cond"].cuda(), method="ddpm", seed=seed, row_offset=roff, **KW)
    inj = m.invert(c["x0"].cuda(), c["cond"].cuda(), method="ddpm", noise=eps.cuda(), **KW)
    assert_close(gen.x_start, inj.x_start, RTOL, ATOL, "generated vs injected: x_start")
    assert_close(_cz(gen.noise, c["coef"]), _cz(inj.noise, c["coef"]), RTOL, ATOL, "generated vs injected: C z")
    other = m.invert(c["x0"].cuda(), c["cond"].cuda(), method="ddpm", seed=seed + 1, row_offset=roff, **KW)
    assert not torch.equal(other.x_start, gen.x_start)


# ---- 6. - 8. launch groups, shards, repeats: equal bits --------------------------------------------------------------------------
def _option(m, name):
    v = C.c_int64(-1)
    L.check(L.lib().osd_get_option(m._engine().handle, name, C.byref(v)))
    return int(v.value)


def test_group_boundaries_shards_and_repeats_bit_for_bit():
    c = _case("epsilon")
    m = c["m"]
    xd, cd = c["x0"].cuda(), c["cond"].cuda()
    kw = dict(method="ddpm", seed=13, **KW)
    whole = m.invert(xd, cd, **kw)
    again = m.invert(xd, cd, **kw)
    assert torch.equal(whole.x_start, again.x_start) and torch.equal(whole.noise, again.noise), "two calls on the same inputs"
    default = _option(m, b"bound_rows")
    assert default >= (S - 1) * N                                # the runs above were one launch group
    m.bound_rows = 700                                           # 2 700 rows: groups of 700 end inside a level (300 rows each)
    try:
        cut = m.invert(xd, cd, **kw)
        assert _option(m, b"bound_rows") == 700
    finally:
        m.bound_rows = default
    assert torch.equal(cut.x_start, whole.x_start) and torch.equal(cut.noise, whole.noise), "bound_rows = 700 vs the default grouping"
    injected = m.invert(xd, cd, method="ddpm", noise=c["eps"].cuda(), **KW)      # after the capped run: the default grouping again
    assert torch.equal(injected.x_start, c["rec"].x_start) and torch.equal(injected.noise, c["rec"].noise)
    k = 128
    lo = m.invert(xd[:k].contiguous(), cd[:k].contiguous(), row_offset=0, **kw)
    hi = m.invert(xd[k:].contiguous(), cd[k:].contiguous(), row_offset=k, **kw)
    assert torch.equal(torch.cat([lo.x_start, hi.x_start]), whole.x_start), "two shards at row 128: x_start"
    assert torch.equal(torch.cat([lo.noise, hi.noise], dim=1), whole.noise), "two shards at row 128: draws"
    unshifted = m.invert(xd[k:].contiguous(), cd[k:].contiguous(), row_offset=0, **kw)
    assert not torch.equal(unshifted.x_start, hi.x_start), "row_offset must enter the draws"


# ---- 9. the round trip through the chain -------------------------------------------------------------------------------------------
def _chain_steps(m, cond, x_T, zs, taus, coef):
    """osd_sample_chain_steps on the per-layer kernels with the plan as given."""
    eng = m._engine()
    n = x_T.shape[0]
    out = torch.empty_like(x_T)
    flags = L.OSD_F_GRAPH
    L.check(L.lib().osd_sample_chain_steps(eng.handle, L.ptr(cond), n, L.ptr(x_T), L.ptr(zs), 0, 0, L.ptr(out), None, flags, taus.ctypes.data,
                                           coef.ctypes.data, int(taus.size)))
    torch.cuda.synchronize()
    return out


def _replay32(c, first_row):
    """The replay of the device's own x_start and draws in float32 on the CPU: the oracle's denoiser cast to float32."""
    m, coef = c["m"], c["coef"]
    den = oracle_denoiser(O, _sd(m), c["cond"], c["taus"], m.num_steps, len(FULL_H), dtype=torch.float32)
    z = c["rec"].noise.detach().cpu()
    cz = [z[k] * float(coef[S - 1 - k, 2]) for k in range(S - 1)]
    return replay(c["rec"].x_start.detach().cpu(), cz, torch.from_numpy(coef), den, first_row=first_row)[0]


def test_round_trip_returns_the_patient_at_level_0():
    """The chain on the map's plan -- row 0 replaced by the identity row -- from x_start with the map's draws returns y_0.  Errors grow
    along the replay with the product of the A_s, so the tolerance is not derived: the same replay in float32 on the CPU is measured
    against y_0 and the device is allowed 4 times that (the MFMA GEMMs sum in another order) plus ATOL.  Both figures are printed;
    measured: CPU float32 2.07e-5, device 1.46e-5, at max|y_0| = 4.83."""
    c = _case("epsilon")
    m, y0 = c["m"], c["y"][0]
    ident = c["coef"].copy()
    ident[0] = (1.0, 0.0, 0.0, 0.0)
    got = _chain_steps(m, c["cond"].cuda(), c["rec"].x_start, c["rec"].noise, c["taus"], ident)
    err32 = (_replay32(c, (1.0, 0.0)).double() - y0).abs().max().item()
    err = (got.cpu().double() - y0).abs().max().item()
    print(f"round trip: CPU float32 replay {err32:.3e}, device {err:.3e}, max|y_0| {y0.abs().max().item():.3e}")
    assert torch.isfinite(got).all() and err32 > 0
    assert err <= 4 * err32 + ATOL, f"device {err:.3e} > 4 x {err32:.3e} + {ATOL}"
    other = _chain_steps(m, c["cond"].flip(0).contiguous().cuda(), c["rec"].x_start, c["rec"].noise, c["taus"], ident)
    assert (other.cpu().double() - y0).abs().max().item() > 4 * err32 + ATOL, "another condition must leave the tolerance"


# ---- 10. DDIM inversion and edit against float64 -----------------------------------------------------------------------------------
def _decode64(m, cond, x, levels, eta, cz=None):
    """The DDIM chain over ``levels`` in float64, unfolded (test_gpu_ddim.py's ddim_oracle with the draws given as C z)."""
    abar = m.alphas_cumprod.detach().cpu().double()
    den = oracle_denoiser(O, _sd(m), cond, levels, m.num_steps, len(FULL_H))
    n_s = len(levels)
    for s in reversed(range(n_s)):
        a = abar[int(levels[s])]
        ap = abar[int(levels[s - 1])] if s > 0 else torch.tensor(1.0, dtype=torch.float64)
        eps = den(x, s)
        x0 = (x - torch.sqrt(1 - a) * eps) / torch.sqrt(a)
        sigma = eta * torch.sqrt((1 - ap) / (1 - a)) * torch.sqrt(1 - a / ap)
        x = torch.sqrt(ap) * x0 + torch.sqrt(torch.clamp(1 - ap - sigma ** 2, min=0.0)) * eps
        if s > 0 and cz is not None:
            x = x + cz[n_s - 1 - s]
    return x


def test_ddim_inversion_and_edit_against_fp64():
    c = _case("epsilon")
    m = c["m"]
    xd, cd = c["x0"].cuda(), c["cond"].cuda()
    new = c["cond"].flip(0).contiguous()
    abar = m.alphas_cumprod.detach().cpu().double()
    den = oracle_denoiser(O, _sd(m), c["cond"], LEVELS, m.num_steps, len(FULL_H))
    up = ddim_inversion_oracle(abar, LEVELS, c["x0"].double(), den)
    recs = {}
    try:
        for engine, (sampler, variant) in {"layers_graph": ("graph", None), "workspace": ("chain", "workspace")}.items():
            m.sampler, m.chain_variant = sampler, variant
            recs[engine] = m.invert(xd, cd, method="ddim", num_inference_steps=PLAN, strength=STRENGTH)
            assert m.last_sampler == sampler, (engine, m.last_sampler)
    finally:
        m.sampler, m.chain_variant = "graph", None
    rec = recs["layers_graph"]
    assert rec.noise is None and rec.eta == 0.0 and rec.method == "ddim" and np.array_equal(rec.timesteps, LEVELS)
    assert_close(rec.x_start, up, RTOL, ATOL, "invert(method='ddim')")
    assert torch.equal(recs["workspace"].x_start, rec.x_start), "the workspace chain kernel vs the per-layer kernels"
    # edit = invert + decode, both methods
    got = m.edit(xd, cd, new.cuda(), method="ddim", num_inference_steps=PLAN, strength=STRENGTH)
    assert_close(got, _decode64(m, new, up, LEVELS, 0.0), RTOL, ATOL, "edit(method='ddim')")
    got = m.edit(xd, cd, new.cuda(), method="ddpm", noise=c["eps"].cuda(), **KW)
    ref = _decode64(m, new, c["y"][-1], LEVELS, ETA, c["cz"])
    assert_close(got, ref, RTOL, ATOL, "edit(method='ddpm')")
    # sample(timesteps=...) is the replay edit() runs
    same = m.sample(new.cuda(), N, x_T=c["rec"].x_start, noise=c["rec"].noise, timesteps=LEVELS, eta=ETA)
    assert torch.equal(same, got)


# ---- 11. model.edit and generator.counterfactual -----------------------------------------------------------------------------------
def test_edit_under_the_same_condition_returns_the_models_x0_at_level_0():
    c = _case("epsilon")
    m, coef = c["m"], c["coef"]
    x0hat = float(coef[0, 0]) * c["y"][0] + float(coef[0, 1]) * c["outs"][0]
    err32 = (_replay32(c, None).double() - x0hat).abs().max().item()
    got = m.edit(c["x0"].cuda(), c["cond"].cuda(), c["cond"].cuda(), method="ddpm", noise=c["eps"].cuda(), **KW)
    err = (got.cpu().double() - x0hat).abs().max().item()
    print(f"edit, same condition: CPU float32 replay {err32:.3e}, device {err:.3e}, max|x0^| {x0hat.abs().max().item():.3e}")
    assert torch.isfinite(got).all()
    assert err <= 4 * err32 + ATOL
    # near the input: x0^ - x0 = (b_0 / a_0) (eps_0 - out_0) for an epsilon model
    a0, b0 = float(m.sqrt_alphas_cumprod[0]), float(m.sqrt_one_minus_alphas_cumprod[0])
    bound = b0 / a0 * (c["eps"][0].abs().max().item() + c["outs"][0].abs().max().item())
    assert (got.cpu().double() - c["x0"].double()).abs().max().item() <= bound + 4 * err32 + ATOL
    changed = m.edit(c["x0"].cuda(), c["cond"].cuda(), c["cond"].flip(0).contiguous().cuda(), method="ddpm", noise=c["eps"].cuda(), **KW)
    assert (changed - got).abs().max().item() > 4 * err32 + ATOL


def test_generator_counterfactual():
    c = _case("epsilon")
    m = c["m"]
    conf = config(FULL_H, T=T)
    md, ed, pd_ = m.mutation_dim, m.expression_dim, m.pathway_dim
    rs = np.random.default_rng(5)
    n = 96
    feats = np.concatenate([rs.integers(0, 2, (n, md)), np.where(rs.random((n, ed)) < 0.3, 0.0, np.exp(rs.normal(1, 1, (n, ed)))),
                            rs.normal(1, 2, (n, pd_))], axis=1).astype(np.float32)
    cond = rs.normal(size=(n, 3)).astype(np.float32)
    cond[:, 2] = 0.0
    saved = m.feature_transform, m.null_condition, m.input_splitk
    try:
        m.feature_transform = FeatureTransform.fit(feats, {"mutations": md, "expression": ed, "pathways": pd_},
                                                   {"expression": "quantile_normal", "pathways": "standard"}, n_quantiles=64)
        gen = SyntheticPatientGenerator(m, conf, device="cuda")
        kw = dict(sampling_steps=PLAN, strength=0.6, seed=3)
        out = gen.counterfactual(feats, cond, {"metastasis_at_diagnosis": 1}, keep={"mutations": True}, **kw)
        assert set(out) == {"mutations", "expression", "pathways", "conditions", "original_conditions"}
        assert np.array_equal(out["original_conditions"], cond)
        assert np.array_equal(out["conditions"][:, :2], cond[:, :2]) and (out["conditions"][:, 2] == 1).all()
        assert np.array_equal(out["mutations"], feats[:, :md]), "kept columns come back exactly"
        ex = feats[:, md:md + ed]
        assert np.isfinite(out["expression"]).all() and np.isfinite(out["pathways"]).all()
        assert (out["expression"] >= ex.min(0)[None, :]).all() and (out["expression"] <= ex.max(0)[None, :]).all(), "data units, observed range"
        again = gen.counterfactual(feats, cond, {"metastasis_at_diagnosis": 1}, keep={"mutations": True}, **kw)
        assert all(np.array_equal(out[k], again[k]) for k in out)
        rows = gen.counterfactual(feats, cond, new_conditions=out["conditions"], keep={"mutations": True}, **kw)
        assert all(np.array_equal(out[k], rows[k]) for k in out), "scenario and the full rows it stands for"
        same = gen.counterfactual(feats, cond, new_conditions=cond, keep={"mutations": True}, **kw)
        assert not np.array_equal(same["expression"], out["expression"]), "a changed condition changes the patient"
        mask = np.zeros(md + ed + pd_, dtype=bool)
        mask[md:md + 7] = True
        kept = gen.counterfactual({"mutations": feats[:, :md], "expression": ex, "pathways": feats[:, md + ed:]}, cond,
                                  {"metastasis_at_diagnosis": 1}, keep=mask, **kw)
        assert np.array_equal(kept["expression"][:, :7], ex[:, :7]) and not np.array_equal(kept["expression"][:, 7:], ex[:, 7:])
        # guidance and bounds route the decode through the guided / clipped chains
        m.null_condition = [0.0, 0.0, 0.0]
        m.last_sampler = None
        lo, hi = 0.5, 20.0
        b = gen.counterfactual(feats, cond, {"metastasis_at_diagnosis": 1}, guidance_scale=2.0, x0_bounds={"expression": (lo, hi)}, **kw)
        assert m.last_sampler == "graph"
        # data units: inside the bounds up to the round trip of the bound itself through the quantile map (two interpolations: a few fp32
        # roundings of values below 32), as generate(x0_bounds=...) under a transform
        slack = 32 * 2.0 ** -20
        assert (b["expression"] >= lo - slack).all() and (b["expression"] <= hi + slack).all()
        assert not np.array_equal(b["expression"], out["expression"])
        # without a transform the clamp is the last operation on the value: every returned value lies inside the bounds exactly
        m.feature_transform, m.last_sampler = None, None
        plain = SyntheticPatientGenerator(m, conf, device="cuda")
        b = plain.counterfactual(feats, cond, {"metastasis_at_diagnosis": 1}, guidance_scale=2.0,
                                 x0_bounds={"expression": (lo, hi), "pathways": (-1.0, None)}, **kw)
        assert m.last_sampler == "graph"
        assert (b["expression"] >= lo).all() and (b["expression"] <= hi).all() and (b["pathways"] >= -1.0).all()
        assert (b["expression"] == lo).any() or (b["expression"] == hi).any(), "the bounds bind somewhere"
        for bad in (dict(), dict(scenario={"metastasis_at_diagnosis": 1}, new_conditions=cond)):
            with pytest.raises(ValueError, match="exactly one"):
                gen.counterfactual(feats, cond, **bad)
        with pytest.raises(ValueError):
            gen.counterfactual(feats, cond, {"tumour_size": 3})
    finally:
        m.feature_transform, m.null_condition, m.input_splitk = saved


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    c = _case("epsilon")
    m = c["m"]
    xd, cd = c["x0"][:8].cuda(), c["cond"][:8].cuda()
    with pytest.raises(ValueError, match="eta"):
        m.invert(xd, cd, method="ddpm", eta=0.0)
    for strength in (0.0, 1.5):
        with pytest.raises(ValueError, match="strength"):
            m.invert(xd, cd, strength=strength)
        with pytest.raises(ValueError, match="strength"):
            m.edit(xd, cd, cd, method="ddim", strength=strength)
    with pytest.raises(ValueError, match="method"):
        m.invert(xd, cd, method="null_text")
    m.precision = "bf16x3"
    try:
        with pytest.raises(ValueError, match="bf16x3"):
            m.invert(xd, cd, method="ddpm")
    finally:
        m.precision = None
    with pytest.raises(RuntimeError, match="noise"):
        m.invert(xd, cd, method="ddpm", noise=torch.zeros(S - 1, 8, m.data_dim, device="cuda"), **KW)
    with pytest.raises(ValueError, match="strictly increase"):
        m.sample(cd, 8, timesteps=[0, 9, 9])
    linked = _model("sample", seed=3)
    linked.mutation_link = "logistic"
    for method in ("ddpm", "ddim"):
        with pytest.raises(ValueError, match="mutation_link"):
            linked.invert(xd, cd, method=method)
    out = m.invert(xd, cd, method="ddpm", **KW)      # and the handle still works
    assert bool(torch.isfinite(out.noise).all())


def test_c_entry_point_refusals():
    lib = L.lib()
    rh = RawHandle()      # T = 10, D = 40, no schedule, no weights: every case below is refused before anything is read
    try:
        buf = torch.zeros(64, device="cuda")
        p = L.ptr(buf)
        good_t = (C.c_int32 * 3)(0, 5, 9)
        good_c = (C.c_float * 12)(1, -1, 0, 0, 1, -1, .5, 0, 1, -1, .5, 0)

        def call(n=2, t=good_t, coef=good_c, S_=3, roff=0, x=p, xs=p, z=p):
            return lib.osd_noise_map(rh.h, x, p, n, t, coef, S_, None, 1, roff, xs, z)

        def coefs(**at):
            v = list(good_c)
            for k, val in at.items():
                v[int(k[1:])] = val
            return (C.c_float * 12)(*v)

        assert call(x=None) == L.OSD_EINVAL and b"null" in lib.osd_last_error()
        assert call(xs=None) == L.OSD_EINVAL and call(z=None) == L.OSD_EINVAL and call(t=None) == L.OSD_EINVAL and call(coef=None) == L.OSD_EINVAL
        assert call(n=0) == L.OSD_EINVAL
        assert call(S_=0) == L.OSD_EINVAL and call(S_=11) == L.OSD_EINVAL
        assert call(t=(C.c_int32 * 3)(0, 5, 5)) == L.OSD_EINVAL and b"strictly increase" in lib.osd_last_error()
        assert call(t=(C.c_int32 * 3)(5, 0, 9)) == L.OSD_EINVAL
        assert call(t=(C.c_int32 * 3)(0, 5, 10)) == L.OSD_EINVAL and call(t=(C.c_int32 * 3)(-1, 5, 9)) == L.OSD_EINVAL
        assert call(coef=coefs(i4=float("nan"))) == L.OSD_EINVAL and call(coef=coefs(i9=float("inf"))) == L.OSD_EINVAL
        assert call(coef=coefs(i2=0.1)) == L.OSD_EINVAL and b"C_0" in lib.osd_last_error()
        assert call(coef=coefs(i6=0.0)) == L.OSD_EINVAL and b"eta > 0" in lib.osd_last_error()
        assert call(coef=coefs(i10=-0.5)) == L.OSD_EINVAL
        assert call(roff=(1 << 32) - 1) == L.OSD_EINVAL and b"row id space" in lib.osd_last_error()
        assert call(roff=-1) == L.OSD_EINVAL
        assert call() == L.OSD_ESTATE and b"osd_set_schedule" in lib.osd_last_error()      # arguments fine, handle not ready
    finally:
        rh.close()


def test_c_entry_point_state_refusals():
    """An armed one-shot is refused and stays armed; a linked handle and "precision" 1 are refused."""
    lib = L.lib()
    m = _model("sample", seed=4)
    g = torch.Generator().manual_seed(2)
    xd, cd = torch.rand(16, m.data_dim, generator=g).cuda(), torch.randn(16, 3, generator=g).cuda()
    eng = m._engine()
    taus, coef = _plan(m)
    xs, z = torch.empty_like(xd), torch.empty(S - 1, 16, m.data_dim, device="cuda")

    def call():
        return lib.osd_noise_map(eng.handle, L.ptr(xd), L.ptr(cd), 16, taus.ctypes.data, coef.ctypes.data, S, None, 1, 0, L.ptr(xs), L.ptr(z))

    idx = torch.arange(16, device="cuda")
    L.check(lib.osd_train_batch_source(eng.handle, L.ptr(xd), xd.stride(0), L.ptr(cd), cd.stride(0), L.ptr(idx), None, 1.0))
    assert call() == L.OSD_ESTATE and b"armed" in lib.osd_last_error()
    loss = torch.empty(1, device="cuda")      # still armed: a training call without rows of its own takes them from the source
    t32 = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.osd_train_loss_fwd_bwd(eng.handle, None, None, 16, L.ptr(t32), None, None, 1, 0, 0, L.ptr(loss), None, 1.0, None, 0) == L.OSD_OK
    torch.cuda.synchronize()
    assert np.isfinite(loss.item())
    assert call() == L.OSD_OK, L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all())
    L.check(lib.osd_set_output_link(eng.handle, m.mutation_dim))
    try:
        assert call() == L.OSD_EUNSUPPORTED and b"output link" in lib.osd_last_error()
    finally:
        L.check(lib.osd_set_output_link(eng.handle, 0))
    L.check(lib.osd_set_option(eng.handle, b"precision", 1))
    try:
        assert call() == L.OSD_EUNSUPPORTED and b"fp32" in lib.osd_last_error()
    finally:
        L.check(lib.osd_set_option(eng.handle, b"precision", 0))
    assert call() == L.OSD_OK, L.last_error()
    torch.cuda.synchronize()


# ---- 13. no leaked state -----------------------------------------------------------------------------------------------------------
def test_no_leaked_state():
    """osd_bound_sweep, a training call and a plain sample before and after the two inversions.  The sweep and the sampler have no float
    atomics and return the same bits.  The training loss is one float that the workgroups of its launch add up atomically, in whatever
    order they finish: equal inputs give sums that differ by the reordering of at most W partials, each rounding at most 2^-24 of
    the (non-negative) running sum -- W <= 32 feature slots x 3 row tiles x 4 waves = 384 -- so that is what 'unchanged' means there."""
    c = _case("epsilon")
    m = c["m"]
    xd, cd = c["x0"].cuda(), c["cond"].cuda()

    def others():
        bound = m.variational_bound(xd, cd, timesteps=[0, 9, 50], seed=4)["sq_error"]
        m.train()
        try:
            loss = m(xd, cd, t=torch.full((N,), 7, device="cuda"), seed=5).detach().clone()
        finally:
            m.eval()
        return bound, loss, m.sample(cd, N, seed=21)

    before = others()
    m.invert(xd, cd, method="ddpm", seed=9, **KW)
    m.invert(xd, cd, method="ddim", num_inference_steps=PLAN, strength=STRENGTH)
    after = others()
    assert torch.equal(before[0], after[0]), "osd_bound_sweep"
    assert torch.equal(before[2], after[2]), "sample"
    assert abs(before[1].item() - after[1].item()) <= 384 * 2.0 ** -24 * abs(before[1].item()), "osd_train_loss_fwd_bwd"


# ---- 14. counterfactual_consistency --------------------------------------------------------------------------------------------------
def test_counterfactual_consistency():
    """Two real groups that differ by a known shift on four features and nothing else (the cases are the controls' rows, shifted), a
    'counterfactual' that is the original plus that shift: the paired shift IS the real difference.  Host float64 over the kernels'
    double sums of fp32 values: the correlation is 1 to the rounding of those sums."""
    rs = np.random.default_rng(8)
    blocks = {"mutations": 6, "expression": 40, "pathways": 4}
    half, D = 60, 50
    base = np.concatenate([rs.integers(0, 2, (half, 6)), rs.normal(2, 1.5, (half, 40)), rs.normal(0, 1, (half, 4))], axis=1).astype(np.float32)
    shift = np.zeros(D, dtype=np.float32)
    shift[[8, 17, 30, 47]] = (1.5, -2.0, 0.75, 1.0)
    real = np.concatenate([base, base + shift[None, :]])
    real_cond = np.stack([rs.normal(size=2 * half), np.r_[np.zeros(half), np.ones(half)]], axis=1)
    original = base[:40]
    val = BiologicalValidator({"evaluation": {}})
    out = val.counterfactual_consistency(original, original + shift[None, :], real, real_cond, "metastasis", names=["age", "metastasis"], blocks=blocks)
    assert abs(out["cf_effect_pearson"] - 1.0) < 1e-6 and abs(out["cf_effect_slope"] - 1.0) < 1e-6
    assert out["cf_sign_agreement"] == 1.0 and out["cf_real_hits"] >= 1
    assert out["cf_rows_changed_mutation_share"] == 0.0 and out["cf_mean_abs_shift"] > 0
    neg = val.counterfactual_consistency(original, original - shift[None, :], real, real_cond, 1, blocks=blocks)
    assert abs(neg["cf_effect_pearson"] + 1.0) < 1e-6 and neg["cf_sign_agreement"] == 0.0
    flipped = original.copy()
    flipped[:10, 0] = 1 - flipped[:10, 0]
    out = val.counterfactual_consistency(original, flipped, real, real_cond, 1, blocks=blocks)
    assert out["cf_rows_changed_mutation_share"] == 0.25
    with pytest.raises(ValueError):
        val.counterfactual_consistency(original, original[:5], real, real_cond, 1)
    with pytest.raises(ValueError):
        val.counterfactual_consistency(original, original, real, real_cond, "survival", names=["age", "metastasis"])
