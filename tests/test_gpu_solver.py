"""GPU: the DPM-Solver++(2M) multistep sampler (osd_sample_chain_multistep, model.sample(solver="dpmpp_2m"), timestep_spacing=, the
generator's keywords) against the float64 restatement of tests/test_solver_cpu.py: at the chain tolerance, apart from the three wrong
chains, inside the bounds exactly, on the padded state, independent of chunks and shards, and leaving today's calls their bits."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator, _lib as L
from osteosarcoma_diffusionmodel_amd.cvae import BiologyConstrainedVAE
from osteosarcoma_diffusionmodel_amd.ddim import ddim_timesteps, dpmpp_2m_table, known_level_table, logsnr_timesteps
from helpers import FULL_H, SM, SM_H, assert_close, config
from test_gpu_clip import check_inside
from test_gpu_ddim import _model, _run, _use
from test_gpu_known import C0_NONZERO, eps_guided
from test_known_cpu import ATOL, MD, N, PLAN, RTOL, T, make_case, make_known, model_sd, tol_of
from test_clip_cpu import mixed_bounds
from test_solver_cpu import VARIANTS, dpmpp_chain

pytestmark = pytest.mark.gpu

S = 10


def chain_multistep(m, cond, lo, hi, taus, *, x_T=None, zs=None, seed=0, row_offset=0, null=None, w=1.0, known=None, expect=L.OSD_OK):
    """osd_sample_chain_multistep through ctypes on the model's handle: (x_out, mutation mask).  lo = hi = None: unbounded."""
    eng = m._engine()
    n = cond.shape[0]
    out = torch.empty(n, m.data_dim, device="cuda")
    mask = torch.empty(n, m.mutation_dim, device="cuda")
    tau, x0c, hist = dpmpp_2m_table(m.alphas_cumprod, taus)
    level = None if known is None else known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, tau)
    c0 = None if null is None else (C.c_float * len(null))(*null)
    flags = (L.OSD_F_TRAIN_MODE if m.training else 0) | (L.OSD_F_GRAPH if m.use_graph else 0)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float32)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float32)
    rc = L.lib().osd_sample_chain_multistep(eng.handle, L.ptr(cond), n, L.ptr(x_T), L.ptr(zs), seed, row_offset, L.ptr(out), L.ptr(mask), flags,
                                            tau.ctypes.data, x0c.ctypes.data, hist.ctypes.data, None if level is None else level.ctypes.data,
                                            int(tau.size), c0, w, L.ptr(known), m.data_dim,
                                            None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data)
    assert rc == expect, (rc, L.last_error())
    torch.cuda.synchronize()
    return out, mask


@pytest.fixture(scope="module")
def case():
    m = _model()
    c = make_case(m)
    c["sd64"] = model_sd(m, torch.float64)
    c["lo"], c["hi"] = mixed_bounds()
    c["refs"] = {}
    yield m, c
    m.prediction_type = "epsilon"


def plan_ref(case_, bounded, variant=None):
    m, c = case_
    key = (bounded, variant)
    if key not in c["refs"]:
        lo, hi = (c["lo"], c["hi"]) if bounded else (None, None)
        c["refs"][key] = dpmpp_chain(m, c["cond"], c["x_start"], lambda s: None, PLAN, lo, hi, variant=variant, sd=c["sd64"])
    return c["refs"][key]


# ---- a. against the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounded", [True, False], ids=["mixed_bounds", "unbounded"])
def test_plan_against_fp64_oracle(case, bounded):
    m, c = case
    lo, hi = (c["lo"], c["hi"]) if bounded else (None, None)
    ref = plan_ref(case, bounded)
    tol = tol_of(ref)
    outs = {}
    for engine in ("layers_graph", "layers_eager"):
        _use(m, engine)
        out, mask = chain_multistep(m, c["cond"].cuda(), lo, hi, PLAN, x_T=c["x_start"].cuda())
        assert L.lib().osd_sample_engine(m._engine().handle, -1, 0) == 0
        err = (out.cpu().double() - ref).abs().max().item()
        print(f"{engine} bounded={bounded}: max|ref|={ref.abs().max().item():.3e} tol={tol:.3e} err={err:.3e}")
        assert_close(out, ref, RTOL, ATOL, f"{engine} bounded={bounded}")
        assert bool(torch.isfinite(out).all()) and torch.equal(mask, (out[:, :m.mutation_dim] > 0.5).float())
        if bounded:
            check_inside(out, mask, lo, hi, m.mutation_dim)
        outs[engine] = (out, mask)
    assert torch.equal(outs["layers_graph"][0], outs["layers_eager"][0]) and torch.equal(outs["layers_graph"][1], outs["layers_eager"][1])
    got = outs["layers_graph"][0].cpu().double()
    for v in VARIANTS:                   # the tolerance separates: each wrong chain of the CPU test lies outside it
        if v == "raw_history" and not bounded:
            continue                     # without a clamp the raw history is the history
        d = (got - plan_ref(case, bounded, v)).abs().max().item()
        print(f"  {v}: {d:.3e} ({d / tol:.0f} x tol)")
        assert d > tol, v


# ---- b. model.sample(solver="dpmpp_2m") ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "guided", "known", "x0_bounds", "known_x0_bounds", "logsnr", "v_prediction"])
def test_sample_keyword_against_fp64_oracle(case, mode):
    m, c = case
    n = 160                                        # two row tiles, the second partial
    g = torch.Generator().manual_seed(47)
    cond = c["cond"][:n].contiguous()
    x_T = torch.randn(n, m.data_dim, generator=g)
    zs = torch.randn(S - 1, n, m.data_dim, generator=g)
    _use(m, "layers_graph")
    kw = dict(num_inference_steps=S, solver="dpmpp_2m")
    taus = ddim_timesteps(T, S)
    lo = hi = kn = eps_fn = None
    prediction = "epsilon"
    if mode == "guided":
        eps_fn, kw["guidance_scale"] = eps_guided(3.0, C0_NONZERO), 3.0
    if mode in ("known", "known_x0_bounds"):       # the mutation block plus 30 % of the rest; the draws feed the observed elements only
        kn = make_known(c["x0"][:n], "thirty_percent", seed=31)
        kn[:, :MD] = c["x0"][:n, :MD]
    if mode in ("x0_bounds", "known_x0_bounds"):
        lo, hi = c["lo"], c["hi"]
        kw["x0_bounds"] = (lo, hi)
    if mode == "logsnr":
        taus, kw["timestep_spacing"] = logsnr_timesteps(m.alphas_cumprod, S), "logsnr"
        assert not np.array_equal(taus, ddim_timesteps(T, S))
    if mode == "v_prediction":
        prediction = "v_prediction"
    ref = dpmpp_chain(m, cond, x_T, lambda s: zs[S - 1 - s], taus, lo, hi, eps_fn=eps_fn, known=kn, sd=c["sd64"], prediction=prediction)
    m.prediction_type = prediction
    if mode == "guided":
        m.null_condition = C0_NONZERO
    try:
        out, mask = m.sample(cond.cuda(), n, x_T=x_T.cuda(), noise=None if kn is None else zs.cuda(), known=None if kn is None else kn.cuda(),
                             return_mutation_mask=True, **kw)
    finally:
        m.null_condition = None
        m.prediction_type = "epsilon"
    assert m.last_sampler == "graph"
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"{mode}: max|ref|={ref.abs().max().item():.3e} tol={tol_of(ref):.3e} err={err:.3e}")
    assert_close(out, ref, RTOL, ATOL, mode)
    assert bool(torch.isfinite(out).all()) and torch.equal(mask, (out[:, :m.mutation_dim] > 0.5).float())
    obs = None
    if kn is not None:
        obs = ~torch.isnan(kn).cuda()
        assert torch.equal(out[obs], kn.cuda()[obs])          # observed elements come back bit for bit
        assert bool(obs.any()) and bool((~obs).any())
    if lo is not None:
        check_inside(out, mask, lo, hi, m.mutation_dim, free=None if obs is None else ~obs)


# ---- c. odd dims ---------------------------------------------------------------------------------------------------------------------
def test_unaligned_dims_on_the_padded_state():
    """D = 5142 (D % 4 = 2): device-generated draws on the padded state, whose history rows are Dp wide like the state's, against the
    restatement fed the device's own draws (osd_op_randn), without and with observed values; injected draws with observed values on the
    caller's rows (guarded kernels)."""
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
    x0 = torch.randn(n, D, generator=g)
    x0[:, :dims[0]] = (torch.rand(n, dims[0], generator=g) < 0.3).float()
    kn = torch.full((n, D), float("nan"))
    kn[:, :dims[0]] = x0[:, :dims[0]]
    pick = torch.rand(n, D, generator=g) < 0.1
    kn[pick] = x0[pick]
    kn[:, D - 1] = x0[:, D - 1]                    # the last column, next to the pad
    lo, hi = mixed_bounds(*dims)
    lo[D - 2], hi[D - 2] = -0.5, 0.5               # bounds next to the pad
    seed, off = (7 << 34) + 99, 11
    eng = m._engine()

    def draws(step):
        a = torch.empty(n, D, device="cuda")
        L.check(L.lib().osd_op_randn(eng.handle, L.ptr(a), n, D, seed, off, step, 0))
        return a.cpu()

    noise_T = draws(T)
    zs = {s: draws(s) for s in range(1, len(PLAN))}
    sd64 = model_sd(m, torch.float64)
    for known in (None, kn):
        tag = "free" if known is None else "known"
        ref = dpmpp_chain(m, cond, noise_T, lambda s: zs[s], PLAN, lo, hi, known=known, sd=sd64)
        out, mask = chain_multistep(m, cond.cuda(), lo, hi, PLAN, seed=seed, row_offset=off, known=None if known is None else known.cuda())
        print(f"D={D} {tag}: max|ref|={ref.abs().max().item():.3e} err={(out.cpu().double() - ref).abs().max().item():.3e}")
        assert_close(out, ref, RTOL, ATOL, f"padded state {tag}")
        obs = None if known is None else ~torch.isnan(known).cuda()
        check_inside(out, mask, lo, hi, dims[0], free=None if obs is None else ~obs)
        if known is not None:
            assert torch.equal(out[obs], known.cuda()[obs])
            inj = torch.stack([zs[s] for s in range(len(PLAN) - 1, 0, -1)]).cuda()
            out_i, mask_i = chain_multistep(m, cond.cuda(), lo, hi, PLAN, x_T=noise_T.cuda(), zs=inj, known=known.cuda())
            assert_close(out_i, ref, RTOL, ATOL, "injected draws")
            check_inside(out_i, mask_i, lo, hi, dims[0], free=~obs)
            assert torch.equal(out_i[obs], known.cuda()[obs])


# ---- d. independence, unchanged bits ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def philox_case():
    m = _model(seed=2)
    cond = torch.randn(N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    x0 = torch.randn(N, m.data_dim, generator=torch.Generator().manual_seed(6))
    x0[:, :MD] = (x0[:, :MD] > 0.5).float()
    return m, cond, make_known(x0, "thirty_percent").cuda()


@pytest.mark.parametrize("with_known", [False, True], ids=["free", "known"])
def test_rows_do_not_depend_on_chunk_or_shard(philox_case, with_known):
    m, cond, kn = philox_case
    lo, hi = mixed_bounds()
    kw = dict(seed=13, num_inference_steps=S, solver="dpmpp_2m", x0_bounds=(lo, hi))

    def rows(a, b):
        return dict(known=kn[a:b].contiguous()) if with_known else {}

    try:
        assert m.input_splitk == 0
        whole, whole_mask = _run(m, "layers_graph", cond, N, **kw, **rows(0, N))
        k = 128
        a, ma = _run(m, "layers_graph", cond[:k].contiguous(), k, row_offset=0, **kw, **rows(0, k))
        b, mb = _run(m, "layers_graph", cond[k:].contiguous(), N - k, row_offset=k, **kw, **rows(k, N))
        assert torch.equal(torch.cat([a, b]), whole) and torch.equal(torch.cat([ma, mb]), whole_mask)
        m.sample_chunk_rows = 128
        for engine in ("layers_graph", "layers_eager"):
            chunked, chunked_mask = _run(m, engine, cond, N, **kw, **rows(0, N))
            assert torch.equal(chunked, whole) and torch.equal(chunked_mask, whole_mask), engine
    finally:
        m.sample_chunk_rows = 65536
        m._engine()
        m.sample_chunk_rows = None


def test_other_calls_keep_their_bits(philox_case):
    """solver=None and solver="ddim" are the call without the keyword, on the default engine: DDIM, DDPM, and with bounds."""
    m, cond, _ = philox_case
    m.sampler, m.use_graph, m.chain_variant, m.squad_panel = "auto", True, None, None
    for base in (dict(seed=5, num_inference_steps=S), dict(seed=5, num_inference_steps=S, eta=0.5), dict(seed=5),
                 dict(seed=5, num_inference_steps=S, x0_bounds=(0.0, 1.0))):
        ref, ref_mask = m.sample(cond, N, return_mutation_mask=True, **base)
        engine = m.last_sampler
        for extra in (dict(solver=None), dict(solver="ddim"), dict(solver="ddim", timestep_spacing="uniform")):
            out, mask = m.sample(cond, N, return_mutation_mask=True, **base, **extra)
            assert m.last_sampler == engine
            assert torch.equal(out, ref) and torch.equal(mask, ref_mask), (base, extra)
    # the multistep solver and the other spacing are other results
    two_m = m.sample(cond, N, seed=5, num_inference_steps=S, solver="dpmpp_2m")
    ref = m.sample(cond, N, seed=5, num_inference_steps=S)
    assert not torch.equal(two_m, ref)
    assert not torch.equal(m.sample(cond, N, seed=5, num_inference_steps=S, timestep_spacing="logsnr"), ref)
    # one and two steps are DDIM at eta = 0: the clipped chain's expressions with G for E, at the chain tolerance
    for steps in (1, 2):
        a = m.sample(cond, N, seed=5, num_inference_steps=steps, solver="dpmpp_2m")
        b = m.sample(cond, N, seed=5, num_inference_steps=steps)
        assert (a - b).abs().max().item() <= tol_of(b), steps


# ---- e. routing and errors --------------------------------------------------------------------------------------------------------------
def test_engine_and_errors(philox_case):
    m, cond, kn_dev = philox_case
    eng = m._engine()
    lo, hi = mixed_bounds()

    def option(name):
        v = C.c_int64(0)
        L.check(L.lib().osd_get_option(eng.handle, name, C.byref(v)))
        return int(v.value)

    kw = dict(seed=21, num_inference_steps=S)
    try:
        for engine in ("workspace", "layers_graph"):
            before, before_mask = _run(m, engine, cond, N, **kw)
            _use(m, "workspace")
            n_fb = option(b"chain_fallbacks")
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                out, mask = m.sample(cond, N, seed=22, num_inference_steps=7, solver="dpmpp_2m", x0_bounds=(lo, hi), return_mutation_mask=True)
            assert m.last_sampler == "graph" and m.last_chain_variant is None and option(b"chain_fallbacks") == n_fb
            assert L.lib().osd_sample_engine(eng.handle, -1, 0) == 0
            check_inside(out, mask, lo, hi, m.mutation_dim)
            after, after_mask = _run(m, engine, cond, N, **kw)                  # no leaked state
            assert torch.equal(before, after) and torch.equal(before_mask, after_mask), engine
        # model.sample's own checks
        _use(m, "layers_graph")
        two_m = dict(num_inference_steps=S, solver="dpmpp_2m")
        with pytest.raises(ValueError, match="solver"):
            m.sample(cond, N, num_inference_steps=S, solver="heun")
        with pytest.raises(ValueError, match="num_inference_steps"):
            m.sample(cond, N, solver="dpmpp_2m")
        with pytest.raises(ValueError, match="eta"):
            m.sample(cond, N, eta=0.5, **two_m)
        with pytest.raises(ValueError, match="noise"):
            m.sample(cond, N, noise=torch.zeros(S - 1, N, m.data_dim, device="cuda"), **two_m)
        with pytest.raises(ValueError, match="timestep_spacing"):
            m.sample(cond, N, num_inference_steps=S, timestep_spacing="quadratic")
        with pytest.raises(ValueError, match="timestep_spacing"):
            m.sample(cond, N, timestep_spacing="logsnr")
        with pytest.raises(ValueError):
            m.sample(cond, N, x0_bounds=(1.0, 0.0), **two_m)
        m.precision = "bf16x3"
        try:
            with pytest.raises(ValueError, match="bf16x3"):
                m.sample(cond, N, **two_m)
        finally:
            m.precision = None
        m.sample(cond, N, **two_m)
        # train mode (dropout in the trunk, as in the other chains): inside the bounds, the same bits for the same seed
        m.train()
        try:
            a, am = m.sample(cond, N, seed=9, x0_bounds=(lo, hi), return_mutation_mask=True, **two_m)
            b = m.sample(cond, N, seed=9, x0_bounds=(lo, hi), **two_m)
            assert m.last_sampler == "graph"
            assert torch.equal(a, b)
            check_inside(a, am, lo, hi, m.mutation_dim)
        finally:
            m.eval()
        assert not torch.equal(a, m.sample(cond, N, seed=9, x0_bounds=(lo, hi), **two_m))      # dropout was on
        # the C ABI's own checks, made on the host before any device call: a chain-kernel run first, whose engine record must stay
        _run(m, "workspace", cond, N, **kw)
        assert option(b"last_engine") == 1
        n_fb, variant = option(b"chain_fallbacks"), option(b"last_chain_variant")
        tau, x0c, hist = dpmpp_2m_table(m.alphas_cumprod, ddim_timesteps(T, S))
        level = known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, tau)
        out = torch.empty(N, m.data_dim, device="cuda")
        kn = torch.full((N, m.data_dim), float("nan"), device="cuda")
        kn[:, :MD] = 1.0

        def raw(lo_=lo, hi_=hi, x0c_=x0c, hist_=hist, n_steps=S, null=None, w=1.0, flags=0, known=None, level_=None, ld=None, tau_=tau):
            return L.lib().osd_sample_chain_multistep(eng.handle, L.ptr(cond), N, None, None, 1, 0, L.ptr(out), None, flags,
                                                      None if tau_ is None else tau_.ctypes.data, None if x0c_ is None else x0c_.ctypes.data,
                                                      None if hist_ is None else hist_.ctypes.data, None if level_ is None else level_.ctypes.data,
                                                      n_steps, null, w, L.ptr(known), m.data_dim if ld is None else ld,
                                                      None if lo_ is None else lo_.ctypes.data, None if hi_ is None else hi_.ctypes.data)

        def rejected(rc, code=L.OSD_EINVAL):
            assert rc == code, (rc, L.last_error())
            assert option(b"last_engine") == 1 and option(b"chain_fallbacks") == n_fb and option(b"last_chain_variant") == variant

        rejected(raw(tau_=None))                                               # a solver needs a plan
        rejected(raw(x0c_=None))
        rejected(raw(hist_=None))
        for i, v in ((0, float("inf")), (5, float("nan")), (4 * S - 1, float("-inf"))):      # a non-finite x0_coef
            bad = x0c.copy()
            bad.reshape(-1)[i] = v
            rejected(raw(x0c_=bad))
        for i, v in ((1, float("inf")), (S - 2, float("nan"))):               # a non-finite hist_coef
            bad = hist.copy()
            bad[i] = v
            rejected(raw(hist_=bad))
        for i, v in ((2, 0.5), (3, 0.25)):                                     # x0_coef[0] != (., ., 1, 0)
            bad = x0c.copy()
            bad[0, i] = v
            rejected(raw(x0c_=bad))
        for i in (0, S - 1):                                                   # hist_coef[0] != 0, hist_coef[n_steps - 1] != 0
            bad = hist.copy()
            bad[i] = -0.25
            rejected(raw(hist_=bad))
        # what the clipped, known, guided and steps entry points reject
        rejected(raw(lo_=None))                                                # one NULL bound
        rejected(raw(hi_=None))
        for side in (0, 1):
            b2 = [lo.copy(), hi.copy()]
            b2[side][m.data_dim - 1] = float("nan")
            rejected(raw(lo_=b2[0], hi_=b2[1]))
        b2 = lo.copy()
        b2[7] = 2.0                                                            # lo > hi (hi[7] = 1)
        rejected(raw(lo_=b2))
        rejected(raw(known=kn, level_=None))
        bad = level.copy()
        bad[0, 0] = 0.5
        rejected(raw(known=kn, level_=bad))
        rejected(raw(known=kn, level_=level, ld=m.data_dim - 1))
        rejected(raw(n_steps=0))
        rejected(raw(n_steps=T + 1))
        wrong_tau = tau.copy()
        wrong_tau[3] = T
        rejected(raw(tau_=wrong_tau))
        c0 = (C.c_float * 3)(0.0, float("nan"), 0.0)
        rejected(raw(null=c0, w=3.0))
        c0 = (C.c_float * 3)(*C0_NONZERO)
        rejected(raw(null=c0, w=float("inf")))
        rejected(raw(null=c0, w=3.0, flags=L.OSD_F_TRAIN_MODE))                # a guided chain is eval mode only
        L.check(L.lib().osd_set_option(eng.handle, b"precision", 1))
        try:
            rejected(raw(), L.OSD_EUNSUPPORTED)
        finally:
            L.check(L.lib().osd_set_option(eng.handle, b"precision", 0))
        # ... and what it accepts
        assert raw() == L.OSD_OK and option(b"last_engine") == 0
        assert raw(lo_=None, hi_=None) == L.OSD_OK                             # unbounded
        assert raw(known=kn, level_=level) == L.OSD_OK
        assert raw(null=c0, w=3.0) == L.OSD_OK
        assert raw(flags=L.OSD_F_TRAIN_MODE) == L.OSD_OK
        torch.cuda.synchronize()
    finally:
        m.precision = None
        m.eval()


# ---- f. the generator ---------------------------------------------------------------------------------------------------------------------
def test_generator_surface():
    conf = config(SM_H, T=50)
    torch.manual_seed(4)
    m = BiologyAwareDiffusionModel(config=conf, **SM).cuda().eval()
    gen = SyntheticPatientGenerator(m, conf, device="cuda")
    md, ed, pd_ = SM["mutation_dim"], SM["expression_dim"], SM["pathway_dim"]
    n = 40
    sc = {"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0}
    keys = ("mutations", "expression", "pathways")
    ddim = gen.generate(n, sc, seed=3, sampling_steps=10)
    got = gen.generate(n, sc, seed=3, sampling_steps=10, solver="dpmpp_2m")
    assert m.last_sampler == "graph"
    assert all(np.isfinite(got[k]).all() for k in keys) and not np.array_equal(got["expression"], ddim["expression"])
    # what model.sample returns for the same call
    cond = gen.create_conditions(n, sc)
    direct = m.sample(cond, n, seed=3, num_inference_steps=10, solver="dpmpp_2m").cpu().numpy()
    assert np.array_equal(direct[:, md:md + ed], got["expression"]) and np.array_equal(direct[:, md + ed:], got["pathways"])
    assert np.array_equal(got["mutations"], (direct[:, :md] > 0.5).astype(float))
    same = gen.generate(n, sc, seed=3, sampling_steps=10, solver="ddim", timestep_spacing="uniform")
    assert all(np.array_equal(same[k], ddim[k]) for k in keys)
    log = gen.generate(n, sc, seed=3, sampling_steps=10, solver="dpmpp_2m", timestep_spacing="logsnr")
    assert np.isfinite(log["expression"]).all() and not np.array_equal(log["expression"], got["expression"])
    # the config's generation.solver / generation.timestep_spacing are the defaults
    gen_c = SyntheticPatientGenerator(m, dict(conf, generation={"solver": "dpmpp_2m"}), device="cuda")
    by_conf = gen_c.generate(n, sc, seed=3, sampling_steps=10)
    assert all(np.array_equal(by_conf[k], got[k]) for k in keys)
    over = gen_c.generate(n, sc, seed=3, sampling_steps=10, solver="ddim")
    assert all(np.array_equal(over[k], ddim[k]) for k in keys)
    gen_l = SyntheticPatientGenerator(m, dict(conf, generation={"solver": "dpmpp_2m", "timestep_spacing": "logsnr"}), device="cuda")
    by_conf = gen_l.generate(n, sc, seed=3, sampling_steps=10)
    assert all(np.array_equal(by_conf[k], log[k]) for k in keys)
    with pytest.raises(ValueError):
        gen_c.generate(n, sc, seed=3)              # the solver needs sampling_steps
    with pytest.raises(ValueError):
        gen.generate(n, sc, sampling_steps=10, solver="heun")
    scen = [{"name": "a", "conditions": sc}, {"name": "b", "conditions": dict(sc, event_occurred=1)}]
    for batched in (True, False):
        res = gen.generate_scenarios(scen, n, batched=batched, sampling_steps=10, solver="dpmpp_2m", **({"seed": 3} if batched else {}))
        assert set(res) == {"a", "b"} and all(np.isfinite(res[k]["expression"]).all() for k in res)
        if batched:
            assert np.array_equal(res["a"]["expression"], got["expression"])      # rows [0, n) of the batch are the single call's
    # impute: the observed values are the observed values, and the bounds hold in the holes
    rng = np.random.default_rng(0)
    feats = rng.standard_normal((n, md + ed + pd_)).astype(np.float32)
    feats[:, :md] = (rng.random((n, md)) < 0.4)
    holes = rng.random(feats.shape) < 0.3
    feats_h = np.where(holes, np.nan, feats).astype(np.float32)
    cond_np = rng.standard_normal((n, 3)).astype(np.float32)
    imp = gen.impute(feats_h, cond_np, seed=7, sampling_steps=10, solver="dpmpp_2m", x0_bounds={"expression": (-2, 2)})
    full = np.concatenate([imp["mutations"], imp["expression"], imp["pathways"]], axis=1)
    assert np.array_equal(full[~holes], feats[~holes]) and np.isfinite(full).all()
    assert np.abs(imp["expression"][holes[:, md:md + ed]]).max() <= 2.0
    # a cVAE has no reverse chain to solve
    vconf = {"model": {"latent_dim": 16, "hidden_dims": [32, 64, 32], "gnn": {"dropout": 0.2},
                       "condition_on": conf["model"]["condition_on"],
                       "constraints": {"pathway_coherence_weight": 1.0, "mutation_expression_weight": 0.5, "survival_prediction_weight": 0.3}}}
    vgen = SyntheticPatientGenerator(BiologyConstrainedVAE(md, ed, pd_, 3, vconf), vconf, device="cuda")
    with pytest.raises(ValueError, match="cVAE"):
        vgen.generate(n, sc, solver="dpmpp_2m")
    with pytest.raises(ValueError, match="cVAE"):
        vgen.generate(n, sc, timestep_spacing="logsnr")
    with pytest.raises(ValueError, match="cVAE"):
        vgen.impute(feats_h, cond_np, solver="dpmpp_2m")
