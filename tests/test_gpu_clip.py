"""GPU: clipping of the predicted x0 inside the sampling step (osd_sample_chain_clipped, model.sample(x0_bounds=...), the generator's
x0_bounds=) against the float64 restatement of tests/test_clip_cpu.py: inside the bounds exactly, at the chain tolerance, apart from
the four wrong chains, the unclipped chain where nothing is bounded, and independent of chunks and shards."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator, _lib as L
from osteosarcoma_diffusionmodel_amd.cvae import BiologyConstrainedVAE
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table, ddim_timesteps, ddim_x0_table, known_level_table
from helpers import FULL_H, SM, SM_H, assert_close, config
from test_gpu_ddim import ENGINES, _model, _run, _use
from test_gpu_known import C0_NONZERO, eps_guided
from test_known_cpu import ATOL, MD, N, PLAN, RTOL, T, make_case, make_known, model_sd, tol_of
from test_clip_cpu import ETAS, INF, VARIANTS, clip_chain, mixed_bounds

pytestmark = pytest.mark.gpu

S = 10


def chain_clipped(m, cond, lo, hi, *, x_T=None, zs=None, seed=0, row_offset=0, taus=None, eta=0.0, null=None, w=1.0, known=None,
                  expect=L.OSD_OK):
    """osd_sample_chain_clipped through ctypes on the model's handle: (x_out, mutation mask); taus = None is the DDPM chain."""
    eng = m._engine()
    n = cond.shape[0]
    out = torch.empty(n, m.data_dim, device="cuda")
    mask = torch.empty(n, m.mutation_dim, device="cuda")
    tau = coef = x0c = level = None
    if taus is not None:
        tau, coef = ddim_step_table(m.alphas_cumprod, taus, eta)
        x0c = ddim_x0_table(m.alphas_cumprod, tau, eta)
        if known is not None:
            level = known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, tau)
    c0 = None if null is None else (C.c_float * len(null))(*null)
    flags = (L.OSD_F_TRAIN_MODE if m.training else 0) | (L.OSD_F_GRAPH if m.use_graph else 0)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float32)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float32)
    rc = L.lib().osd_sample_chain_clipped(eng.handle, L.ptr(cond), n, L.ptr(x_T), L.ptr(zs), seed, row_offset, L.ptr(out), L.ptr(mask), flags,
                                          None if tau is None else tau.ctypes.data, None if coef is None else coef.ctypes.data,
                                          None if x0c is None else x0c.ctypes.data, None if level is None else level.ctypes.data,
                                          0 if tau is None else int(tau.size), c0, w, L.ptr(known), m.data_dim,
                                          None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data)
    assert rc == expect, (rc, L.last_error())
    torch.cuda.synchronize()
    return out, mask


def check_inside(out, mask, lo, hi, md, free=None):
    """Every element (of the rows / elements `free` selects) lies inside [lo, hi], no tolerance; the mask is (out > 0.5)."""
    lo_t, hi_t = torch.from_numpy(lo).to(out.device), torch.from_numpy(hi).to(out.device)
    inside = (out >= lo_t) & (out <= hi_t)
    if free is not None:
        inside = inside | ~free
    assert bool(inside.all()), f"{int((~inside).sum())} elements outside the bounds"
    assert bool(torch.isfinite(out).all())
    assert torch.equal(mask, (out[:, :md] > 0.5).float())


@pytest.fixture(scope="module")
def case():
    m = _model()
    c = make_case(m)
    c["sd64"] = model_sd(m, torch.float64)
    c["lo"], c["hi"] = mixed_bounds()
    c["refs"] = {}
    return m, c


def plan_ref(case_, eta, variant=None):
    m, c = case_
    key = (eta, variant)
    if key not in c["refs"]:
        c["refs"][key] = clip_chain(m, c["cond"], c["x_start"], lambda s: c["zs"][len(PLAN) - 1 - s], PLAN, eta, c["lo"], c["hi"],
                                    variant=variant, sd=c["sd64"])
    return c["refs"][key]


# ---- a. against the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("engine", ["layers_graph", "layers_eager"])
def test_plan_against_fp64_oracle(case, engine, eta):
    m, c = case
    _use(m, engine)
    out, mask = chain_clipped(m, c["cond"].cuda(), c["lo"], c["hi"], x_T=c["x_start"].cuda(), zs=c["zs"].cuda(), taus=PLAN, eta=eta)
    assert L.lib().osd_sample_engine(m._engine().handle, -1, 0) == 0
    ref = plan_ref(case, eta)
    tol = tol_of(ref)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"{engine} eta={eta}: max|ref|={ref.abs().max().item():.3e} tol={tol:.3e} err={err:.3e}")
    assert_close(out, ref, RTOL, ATOL, f"{engine} eta={eta}")
    check_inside(out, mask, c["lo"], c["hi"], m.mutation_dim)
    if engine == "layers_graph":         # the tolerance separates: each wrong chain of the CPU test lies outside it
        for v in VARIANTS:
            d = (out.cpu().double() - plan_ref(case, eta, v)).abs().max().item()
            print(f"  {v}: {d:.3e} ({d / tol:.0f} x tol)")
            assert d > tol, v


# ---- b. model.sample(x0_bounds=...) -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ddim", "ddpm", "ddpm_guided", "ddim_known"])
def test_sample_keyword_against_fp64_oracle(case, mode):
    # From pure noise at T = 100 the free and one-sided columns reach |x| ~ 2.5e4 and set the chain tolerance (~1.3) for every column;
    # the five-step plan above, where max|x| ~ 9, is the sharp comparison.  The two-sided columns alone are printed for the record: they
    # see the large columns through eps, so no tighter bound follows for them.
    m, c = case
    n = 160                                        # two row tiles, the second partial
    g = torch.Generator().manual_seed(43)
    cond = c["cond"][:n].contiguous()
    x_T = torch.randn(n, m.data_dim, generator=g)
    lo, hi = c["lo"], c["hi"]
    spec = (lo, hi)
    _use(m, "layers_graph")
    kn = eps_fn = post = None
    if mode in ("ddim", "ddim_known"):
        taus, eta, kw = ddim_timesteps(T, S), 0.0, dict(num_inference_steps=S, eta=0.0)
        n_draws = S - 1
        if mode == "ddim_known":                   # the mutation block plus 30 % of the rest; eta = 0: the draws feed the observed elements only
            kn = make_known(c["x0"][:n], "thirty_percent", seed=31)
            kn[:, :MD] = c["x0"][:n, :MD]
    else:                                          # the DDPM chain: the reference's posterior coefficients, not the DDIM table
        taus, eta, kw = None, 1.0, {}
        n_draws = T - 1
        post = O.posterior_coefficients({"betas": m.betas.detach().cpu(), "alphas_cumprod": m.alphas_cumprod.detach().cpu()})
        eps_fn = eps_guided(3.0, C0_NONZERO) if mode == "ddpm_guided" else None
    zs = torch.randn(n_draws, n, m.data_dim, generator=g) if (mode != "ddim") else None
    ref = clip_chain(m, cond, x_T, (lambda s: zs[n_draws - s]) if zs is not None else (lambda s: torch.zeros(n, m.data_dim)), taus, eta, lo, hi,
                     eps_fn=eps_fn, known=kn, sd=c["sd64"], post=post)
    if mode == "ddpm_guided":
        m.null_condition, kw["guidance_scale"] = C0_NONZERO, 3.0
    try:
        out, mask = m.sample(cond.cuda(), n, x_T=x_T.cuda(), noise=None if zs is None else zs.cuda(), known=None if kn is None else kn.cuda(),
                             x0_bounds=spec, return_mutation_mask=True, **kw)
    finally:
        m.null_condition = None
    assert m.last_sampler == "graph"
    err = (out.cpu().double() - ref).abs().max().item()
    two = torch.from_numpy(np.isfinite(lo) & np.isfinite(hi))
    err_two = (out.cpu().double() - ref)[:, two].abs().max().item()
    print(f"{mode}: max|ref|={ref.abs().max().item():.3e} tol={tol_of(ref):.3e} err={err:.3e} (two-sided columns alone: {err_two:.3e})")
    assert_close(out, ref, RTOL, ATOL, mode)
    if kn is None:
        check_inside(out, mask, lo, hi, m.mutation_dim)
    else:
        obs = ~torch.isnan(kn).cuda()
        assert torch.equal(out[obs], kn.cuda()[obs])          # observed elements come back bit for bit
        check_inside(out, mask, lo, hi, m.mutation_dim, free=~obs)
        assert bool(obs.any()) and bool((~obs).any())


# ---- c. reduction to the unclipped chain ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def philox_case():
    m = _model(seed=2)
    cond = torch.randn(N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    return m, cond


@pytest.mark.parametrize("eta", ETAS)
def test_infinite_bounds_are_the_unclipped_chain(philox_case, eta):
    """All-infinite bounds through the C entry point run the new kernel and agree with the unclipped per-layer chain at the chain
    tolerance (another operation order: no bits expected); through model.sample, None without a model attribute and False with one take
    today's entry points on every engine."""
    m, cond = philox_case
    free_lo, free_hi = np.full(m.data_dim, -INF, dtype=np.float32), np.full(m.data_dim, INF, dtype=np.float32)
    kw = dict(seed=77, row_offset=5, num_inference_steps=S, eta=eta)
    ref, ref_mask = _run(m, "layers_graph", cond, N, **kw)
    out, mask = chain_clipped(m, cond, free_lo, free_hi, seed=77, row_offset=5, taus=ddim_timesteps(T, S), eta=eta)
    d = (out - ref).abs().max().item()
    print(f"eta={eta}: all-infinite bounds against the unclipped chain {d:.3e} (tol {tol_of(ref):.3e})")
    assert d <= tol_of(ref) and bool(torch.isfinite(out).all())
    assert torch.equal(mask, (out[:, :m.mutation_dim] > 0.5).float())
    if eta == 0.0:                                 # ... and the DDPM chain, folded from the posterior coefficients
        ref_d, _ = _run(m, "layers_graph", cond, N, seed=78, row_offset=5)
        out_d, _ = chain_clipped(m, cond, free_lo, free_hi, seed=78, row_offset=5)
        assert (out_d - ref_d).abs().max().item() <= tol_of(ref_d)
    try:
        for engine in ENGINES:
            ref_e, ref_em = _run(m, engine, cond, N, **kw)
            assert m.x0_bounds is None
            out_e, mask_e = _run(m, engine, cond, N, x0_bounds=None, **kw)         # _run asserts the engine that ran
            assert torch.equal(out_e, ref_e) and torch.equal(mask_e, ref_em), engine
            m.x0_bounds = (0.0, 1.0)
            out_e, mask_e = _run(m, engine, cond, N, x0_bounds=False, **kw)
            m.x0_bounds = None
            assert torch.equal(out_e, ref_e) and torch.equal(mask_e, ref_em), engine
        # the attribute alone clips
        m.x0_bounds = (0.0, 1.0)
        out_a, _ = _run(m, "layers_graph", cond, N, **kw)
        assert bool(((out_a >= 0) & (out_a <= 1)).all()) and not torch.equal(out_a, ref)
    finally:
        m.x0_bounds = None


# ---- d. independence -----------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_chunk_or_shard(philox_case):
    m, cond = philox_case
    lo, hi = mixed_bounds()
    kw = dict(seed=13, num_inference_steps=S, eta=0.5, x0_bounds=(lo, hi))
    try:
        whole, whole_mask = _run(m, "layers_graph", cond, N, **kw)
        check_inside(whole, whole_mask, lo, hi, m.mutation_dim)
        k = 128
        a, ma = _run(m, "layers_graph", cond[:k].contiguous(), k, row_offset=0, **kw)
        b, mb = _run(m, "layers_graph", cond[k:].contiguous(), N - k, row_offset=k, **kw)
        assert torch.equal(torch.cat([a, b]), whole) and torch.equal(torch.cat([ma, mb]), whole_mask)
        m.sample_chunk_rows = 128
        for engine in ("layers_graph", "layers_eager"):
            chunked, chunked_mask = _run(m, engine, cond, N, **kw)
            assert torch.equal(chunked, whole) and torch.equal(chunked_mask, whole_mask), engine
    finally:
        m.sample_chunk_rows = 65536
        m._engine()
        m.sample_chunk_rows = None


# ---- e. odd dims ---------------------------------------------------------------------------------------------------------------------
def test_unaligned_dims_on_the_padded_state():
    """D = 5142 (D % 4 = 2): device-generated draws on the padded state, whose bounds rows are Dp wide with (-inf, +inf) pad columns,
    against the restatement fed the device's own draws (osd_op_randn); injected draws on the caller's rows (guarded kernels)."""
    dims, cond_dim, n = (62, 5054, 26), 3, 200
    D = sum(dims)
    assert D % 4 != 0
    sd = O.init_state_dict(O.param_shapes(*dims, cond_dim, FULL_H, 128), seed=33)
    m = BiologyAwareDiffusionModel(*dims, cond_dim, config(FULL_H, T=T))
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.input_splitk = 0
    m.sampler = "graph"
    g = torch.Generator().manual_seed(6)
    cond = torch.randn(n, cond_dim, generator=g)
    lo, hi = mixed_bounds(*dims)
    lo[D - 1], hi[D - 1] = -0.5, 0.5               # bounds on the last column, next to the pad
    seed, off = (7 << 34) + 99, 11
    eng = m._engine()

    def draws(step):
        a = torch.empty(n, D, device="cuda")
        L.check(L.lib().osd_op_randn(eng.handle, L.ptr(a), n, D, seed, off, step, 0))
        return a.cpu()

    noise_T = draws(T)
    zs = {s: draws(s) for s in range(1, len(PLAN))}
    for eta in ETAS:
        ref = clip_chain(m, cond, noise_T, lambda s: zs[s], PLAN, eta, lo, hi)
        out, mask = chain_clipped(m, cond.cuda(), lo, hi, seed=seed, row_offset=off, taus=PLAN, eta=eta)
        print(f"D={D} eta={eta}: max|ref|={ref.abs().max().item():.3e} err={(out.cpu().double() - ref).abs().max().item():.3e}")
        assert_close(out, ref, RTOL, ATOL, f"padded state eta={eta}")
        check_inside(out, mask, lo, hi, dims[0])
        inj = torch.stack([zs[s] for s in range(len(PLAN) - 1, 0, -1)]).cuda() if eta > 0 else None
        out_i, mask_i = chain_clipped(m, cond.cuda(), lo, hi, x_T=noise_T.cuda(), zs=inj, taus=PLAN, eta=eta)
        assert_close(out_i, ref, RTOL, ATOL, f"injected draws eta={eta}")
        check_inside(out_i, mask_i, lo, hi, dims[0])


# ---- f. routing and errors --------------------------------------------------------------------------------------------------------------
def test_engine_and_errors(philox_case):
    m, cond = philox_case
    eng = m._engine()
    lo, hi = mixed_bounds()

    def fallbacks():
        v = C.c_int64(0)
        L.check(L.lib().osd_get_option(eng.handle, b"chain_fallbacks", C.byref(v)))
        return int(v.value)

    kw = dict(seed=21, num_inference_steps=S)
    try:
        for engine in ("workspace", "layers_graph"):
            before, before_mask = _run(m, engine, cond, N, **kw)
            _use(m, "workspace")
            n_fb = fallbacks()
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                out, mask = m.sample(cond, N, seed=22, num_inference_steps=7, eta=0.3, x0_bounds=(lo, hi), return_mutation_mask=True)
            assert m.last_sampler == "graph" and m.last_chain_variant is None and fallbacks() == n_fb
            assert L.lib().osd_sample_engine(eng.handle, -1, 0) == 0
            check_inside(out, mask, lo, hi, m.mutation_dim)
            after, after_mask = _run(m, engine, cond, N, **kw)                  # no leaked state
            assert torch.equal(before, after) and torch.equal(before_mask, after_mask), engine
        _use(m, "layers_graph")
        m.precision = "bf16x3"
        try:
            with pytest.raises(ValueError, match="bf16x3"):
                m.sample(cond, N, num_inference_steps=S, x0_bounds=(lo, hi))
        finally:
            m.precision = None
        with pytest.raises(ValueError):
            m.sample(cond, N, num_inference_steps=S, x0_bounds=(1.0, 0.0))
        with pytest.raises(ValueError):
            m.sample(cond, N, num_inference_steps=S, x0_bounds={"genes": (0, 1)})
        # train mode (dropout in the trunk, as in the unclipped chain): inside the bounds, the same bits for the same seed
        m.train()
        try:
            a, am = m.sample(cond, N, seed=9, num_inference_steps=S, eta=0.5, x0_bounds=(lo, hi), return_mutation_mask=True)
            b = m.sample(cond, N, seed=9, num_inference_steps=S, eta=0.5, x0_bounds=(lo, hi))
            assert m.last_sampler == "graph"
            assert torch.equal(a, b)
            check_inside(a, am, lo, hi, m.mutation_dim)
        finally:
            m.eval()
        assert not torch.equal(a, m.sample(cond, N, seed=9, num_inference_steps=S, eta=0.5, x0_bounds=(lo, hi)))      # dropout was on
        # the C ABI's own checks
        taus = ddim_timesteps(T, S)
        tau, coef = ddim_step_table(m.alphas_cumprod, taus, 0.0)
        x0c = ddim_x0_table(m.alphas_cumprod, tau, 0.0)
        level = known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, tau)
        out = torch.empty(N, m.data_dim, device="cuda")
        kn = torch.full((N, m.data_dim), float("nan"), device="cuda")
        kn[:, :MD] = 1.0

        def raw(lo_=lo, hi_=hi, x0c_=x0c, coef_=coef, n_steps=S, null=None, w=1.0, flags=0, known=None, level_=None, ld=None, tau_=tau):
            return L.lib().osd_sample_chain_clipped(eng.handle, L.ptr(cond), N, None, None, 1, 0, L.ptr(out), None, flags,
                                                    None if tau_ is None else tau_.ctypes.data, coef_.ctypes.data,
                                                    None if x0c_ is None else x0c_.ctypes.data, None if level_ is None else level_.ctypes.data,
                                                    n_steps, null, w, L.ptr(known), m.data_dim if ld is None else ld,
                                                    None if lo_ is None else lo_.ctypes.data, None if hi_ is None else hi_.ctypes.data)

        assert raw() == L.OSD_OK
        assert raw(known=kn, level_=level) == L.OSD_OK
        assert raw(tau_=None, x0c_=None) == L.OSD_OK                           # the DDPM chain: x0_coef ignored
        assert raw(lo_=None) == L.OSD_EINVAL and raw(hi_=None) == L.OSD_EINVAL    # a NULL bound
        for side in (0, 1):
            for i, v in ((3, float("nan")), (m.data_dim - 1, float("nan"))):   # a NaN bound
                b2 = [lo.copy(), hi.copy()]
                b2[side][i] = v
                assert raw(lo_=b2[0], hi_=b2[1]) == L.OSD_EINVAL, (side, i)
        b2 = lo.copy()
        b2[7] = 2.0                                                            # lo > hi (hi[7] = 1)
        assert raw(lo_=b2) == L.OSD_EINVAL
        for i, v in ((0, float("inf")), (5, float("nan")), (4 * S - 1, float("-inf"))):      # a non-finite x0_coef
            bad = x0c.copy()
            bad.reshape(-1)[i] = v
            assert raw(x0c_=bad) == L.OSD_EINVAL, (i, v)
        for i, v in ((2, 0.5), (3, 0.25)):                                     # x0_coef[0] != (., ., 1, 0)
            bad = x0c.copy()
            bad[0, i] = v
            assert raw(x0c_=bad) == L.OSD_EINVAL, (i, v)
        assert raw(x0c_=None) == L.OSD_EINVAL
        # what the known, guided and steps entry points reject
        assert raw(known=kn, level_=None) == L.OSD_EINVAL
        bad = level.copy()
        bad[0, 0] = 0.5
        assert raw(known=kn, level_=bad) == L.OSD_EINVAL
        assert raw(known=kn, level_=level, ld=m.data_dim - 1) == L.OSD_EINVAL
        assert raw(n_steps=0) == L.OSD_EINVAL and raw(n_steps=T + 1) == L.OSD_EINVAL
        wrong = coef.copy()
        wrong[0, 2] = 0.1
        assert raw(coef_=wrong) == L.OSD_EINVAL
        wrong_tau = tau.copy()
        wrong_tau[3] = T
        assert raw(tau_=wrong_tau) == L.OSD_EINVAL
        c0 = (C.c_float * 3)(0.0, float("nan"), 0.0)
        assert raw(null=c0, w=3.0) == L.OSD_EINVAL
        c0 = (C.c_float * 3)(*C0_NONZERO)
        assert raw(null=c0, w=float("inf")) == L.OSD_EINVAL
        assert raw(null=c0, w=3.0, flags=L.OSD_F_TRAIN_MODE) == L.OSD_EINVAL      # a guided chain is eval mode only
        assert raw(null=c0, w=3.0) == L.OSD_OK
        L.check(L.lib().osd_set_option(eng.handle, b"precision", 1))
        try:
            assert raw() == L.OSD_EUNSUPPORTED
        finally:
            L.check(L.lib().osd_set_option(eng.handle, b"precision", 0))
        torch.cuda.synchronize()
    finally:
        m.precision = None
        m.eval()


# ---- g. the generator ---------------------------------------------------------------------------------------------------------------------
def test_generator_surface():
    conf = config(SM_H, T=8)
    torch.manual_seed(4)
    m = BiologyAwareDiffusionModel(config=conf, **SM).cuda().eval()
    gen = SyntheticPatientGenerator(m, conf, device="cuda")
    md, ed, pd_ = SM["mutation_dim"], SM["expression_dim"], SM["pathway_dim"]
    n = 40
    sc = {"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0}
    spec = {"mutations": (0, 1), "expression": (-2, 2)}
    free = gen.generate(n, sc, seed=3)
    got = gen.generate(n, sc, seed=3, x0_bounds=spec)
    assert np.abs(got["expression"]).max() <= 2.0 and np.isfinite(got["pathways"]).all()
    assert not np.array_equal(got["expression"], free["expression"])
    for kw in (dict(sampling_steps=4, eta=0.5), dict(sampling_steps=4)):
        assert np.abs(gen.generate(n, sc, seed=3, x0_bounds=spec, **kw)["expression"]).max() <= 2.0
    # guidance over-shoots by construction; the clamp is its usual remedy
    m.null_condition = [0.3, -0.7, 1.1]
    try:
        loose = gen.generate(n, sc, guidance_scale=7.5, seed=3)
        tight = gen.generate(n, sc, guidance_scale=7.5, seed=3, x0_bounds=spec)
        print(f"guidance 7.5: max|expression| unclipped {np.abs(loose['expression']).max():.3f}, clipped {np.abs(tight['expression']).max():.3f}")
        assert np.abs(loose["expression"]).max() > 2.0           # so that the next line says something
        assert np.abs(tight["expression"]).max() <= 2.0
    finally:
        m.null_condition = None
    # the config's generation.x0_bounds is the default; False switches it off
    conf_b = dict(conf, generation={"x0_bounds": {"mutations": [0, 1], "expression": [-2, 2]}})
    gen_b = SyntheticPatientGenerator(m, conf_b, device="cuda")
    by_conf = gen_b.generate(n, sc, seed=3)
    assert all(np.array_equal(by_conf[k], got[k]) for k in ("mutations", "expression", "pathways"))
    off = gen_b.generate(n, sc, seed=3, x0_bounds=False)
    assert all(np.array_equal(off[k], free[k]) for k in ("mutations", "expression", "pathways"))
    scen = [{"name": "a", "conditions": sc}, {"name": "b", "conditions": dict(sc, event_occurred=1)},
            {"name": "c", "conditions": dict(sc, metastasis_at_diagnosis=1)}]
    for batched in (True, False):
        res = gen.generate_scenarios(scen, n, batched=batched, x0_bounds=spec, **({"seed": 5} if batched else {}))
        assert set(res) == {"a", "b", "c"}
        for name in res:
            assert np.abs(res[name]["expression"]).max() <= 2.0, (batched, name)
        assert not np.array_equal(res["a"]["expression"], res["b"]["expression"])
    # impute with bounds: the observed values are the observed values, the holes stay inside
    rng = np.random.default_rng(0)
    feats = rng.standard_normal((n, md + ed + pd_)).astype(np.float32)
    feats[:, :md] = (rng.random((n, md)) < 0.4)
    holes = rng.random(feats.shape) < 0.3
    feats_h = np.where(holes, np.nan, feats).astype(np.float32)
    cond = rng.standard_normal((n, 3)).astype(np.float32)
    imp = gen.impute(feats_h, cond, seed=7, x0_bounds=spec)
    full = np.concatenate([imp["mutations"], imp["expression"], imp["pathways"]], axis=1)
    assert np.array_equal(full[~holes], feats[~holes]) and np.isfinite(full).all()
    expr_holes = holes[:, md:md + ed]
    assert np.abs(imp["expression"][expr_holes]).max() <= 2.0
    with pytest.raises(ValueError):
        gen.generate(n, sc, x0_bounds={"expression": (2, -2)})
    # a cVAE has no reverse chain to clip in
    vconf = {"model": {"latent_dim": 16, "hidden_dims": [32, 64, 32], "gnn": {"dropout": 0.2},
                       "condition_on": conf["model"]["condition_on"],
                       "constraints": {"pathway_coherence_weight": 1.0, "mutation_expression_weight": 0.5, "survival_prediction_weight": 0.3}}}
    vgen = SyntheticPatientGenerator(BiologyConstrainedVAE(md, ed, pd_, 3, vconf), vconf, device="cuda")
    with pytest.raises(ValueError, match="cVAE"):
        vgen.generate(n, sc, x0_bounds=spec)
    with pytest.raises(ValueError, match="cVAE"):
        vgen.impute(feats_h, cond, x0_bounds=spec)
