"""Host: known-feature conditioning -- the level table (ddim.known_level_table), the observation array (generate.assemble_known) and
a CPU restatement of the chain around observed values, in float64 and float32, with the controls that show the chain tolerance
separates a wrong level, a missing noise term and a missing replacement.  tests/test_gpu_known.py holds the device to the same
float64 restatement."""
import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table, ddim_timesteps, known_level_table
from osteosarcoma_diffusionmodel_amd.generate import assemble_known
from helpers import FULL, FULL_H, config

T, N = 100, 300
PLAN = np.array([5, 20, 35, 50, 65], dtype=np.int32)      # five steps from tau = 65 down: max|x| stays ~10, the tolerance ~5e-4
RTOL, ATOL = 5e-5, 1e-5                                    # the chain tests' tolerance: 5e-5 * max|ref| + 1e-5
ETAS = (0.0, 0.5)
MASKS = ("mutations", "thirty_percent")
VARIANTS = ("level_of_tau_s", "ls_zero", "no_replacement_before_the_last_step")
MD = FULL["mutation_dim"]


def cpu_model(T_=T, seed=0, p=0.2):
    """test_gpu_ddim._model's construction, on the CPU: the same parameters (torch's CPU generator draws them there too)."""
    torch.manual_seed(seed)
    m = BiologyAwareDiffusionModel(config=config(FULL_H, T=T_, p=p), **FULL).eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, prm in m.named_parameters():
            if k.endswith((".1.weight", ".5.weight")):
                prm.copy_(1 + 0.2 * torch.randn(prm.shape, generator=gen))
            if k.endswith((".1.bias", ".5.bias")):
                prm.copy_(0.1 * torch.randn(prm.shape, generator=gen))
    return m


def model_sd(m, dtype):
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.startswith(("condition_embed", "unet"))}
    return O.to_dtype(sd, dtype)


def step_tables(m, taus, eta, dtype):
    """(coef [S][3], level [S][2]) of the plan.  float32: the tables the library is handed (ddim_step_table, known_level_table).
    float64: the same quantities formed in double from the fp32 alphas_cumprod buffer, unfolded as test_gpu_ddim.ddim_oracle does."""
    if dtype == torch.float32:
        _, coef = ddim_step_table(m.alphas_cumprod, taus, eta)
        level = known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, taus)
        return torch.from_numpy(coef[:, :3].copy()), torch.from_numpy(level)
    abar = m.alphas_cumprod.detach().cpu().double()
    coef = torch.zeros(len(taus), 3, dtype=torch.float64)
    level = torch.zeros(len(taus), 2, dtype=torch.float64)
    for s in range(len(taus)):
        a = abar[int(taus[s])]
        ap = abar[int(taus[s - 1])] if s > 0 else torch.tensor(1.0, dtype=torch.float64)
        sigma = eta * torch.sqrt((1 - ap) / (1 - a)) * torch.sqrt(1 - a / ap)
        coef[s, 0] = torch.sqrt(ap / a)
        coef[s, 1] = torch.sqrt(torch.clamp(1 - ap - sigma ** 2, min=0.0)) - torch.sqrt(ap) * torch.sqrt(1 - a) / torch.sqrt(a)
        coef[s, 2] = sigma
        level[s, 0], level[s, 1] = torch.sqrt(ap), torch.sqrt(1 - ap)
    return coef, level


def known_chain(m, cond, x_start, z_of_s, taus, eta, known, dtype=torch.float64, variant=None, eps_fn=None, sd=None):
    """The chain around observed values on the CPU: per step x' = A x + B eps + C z, then the known (non-NaN) elements are
    overwritten with La * known + Ls * z (s > 0; z the step's own draw, z_of_s(s)) or with the observation itself (s = 0).
    variant: one of VARIANTS -- a deliberately wrong chain.  eps_fn(sd, x, t_norm, cond): another denoiser evaluation (guidance)."""
    sd = model_sd(m, dtype) if sd is None else sd
    coef, level = step_tables(m, taus, eta, dtype)
    if variant == "level_of_tau_s":              # the level the step LEAVES, not the one it arrives at
        _, shifted = step_tables(m, np.concatenate([taus[1:], taus[-1:]]), eta, dtype)
        level = torch.cat([level[:1], shifted[1:]])
    cond = cond.detach().cpu().to(dtype)
    x = x_start.detach().cpu().to(dtype)
    kn = known.detach().cpu().to(dtype)
    obs = ~torch.isnan(kn)
    c_emb = O.condition_embed(sd, cond)
    n_s = len(taus)
    for s in reversed(range(n_s)):
        t_norm = torch.full((x.shape[0],), int(taus[s]) / m.num_steps, dtype=dtype)
        if eps_fn is None:
            eps = O.unet_forward(sd, x, t_norm, c_emb, len(FULL_H), 128, None, 0.0)
        else:
            eps = eps_fn(sd, x, t_norm, cond)
        z = z_of_s(s).detach().cpu().to(dtype) if s > 0 else None
        x = coef[s, 0] * x + coef[s, 1] * eps
        if s > 0 and float(coef[s, 2]) != 0.0:
            x = x + coef[s, 2] * z
        if s == 0:
            x = torch.where(obs, kn, x)
        elif variant != "no_replacement_before_the_last_step":
            ls = 0.0 if variant == "ls_zero" else level[s, 1]
            x = torch.where(obs, level[s, 0] * kn + ls * z, x)
    return x


def make_known(x0, which, seed=23):
    """The two observation patterns of the tests, values from the patient x0: the mutation block (0 / 1), or 30 % of all elements."""
    kn = torch.full_like(x0, float("nan"))
    if which == "mutations":
        kn[:, :MD] = x0[:, :MD]
    else:
        pick = torch.rand(x0.shape, generator=torch.Generator().manual_seed(seed)) < 0.3
        kn[pick] = x0[pick]
    return kn


def make_case(m):
    """Inputs of the five-step plan: patients x0 (0 / 1 mutations, normal expression and pathway values), the start
    x = sqrt(abar_65) x0 + sqrt(1 - abar_65) e, conditions and one injected draw per step."""
    g = torch.Generator().manual_seed(11)
    n, D = N, m.data_dim
    cond = torch.randn(n, 3, generator=g)
    x0 = torch.randn(n, D, generator=g)
    x0[:, :MD] = (torch.rand(n, MD, generator=g) < 0.3).float()
    e = torch.randn(n, D, generator=g)
    zs = torch.randn(len(PLAN) - 1, n, D, generator=g)
    a = m.alphas_cumprod.detach().cpu()[int(PLAN[-1])]
    x_start = torch.sqrt(a) * x0 + torch.sqrt(1 - a) * e
    return dict(cond=cond, x0=x0, x_start=x_start, zs=zs, known={k: make_known(x0, k) for k in MASKS})


def tol_of(ref):
    return ATOL + RTOL * ref.abs().max().item()


@pytest.fixture(scope="module")
def chains():
    m = cpu_model()
    c = make_case(m)
    sd64, sd32 = model_sd(m, torch.float64), model_sd(m, torch.float32)
    out = {}
    for eta in ETAS:
        for which in MASKS:
            def run(dtype, variant=None):
                return known_chain(m, c["cond"], c["x_start"], lambda s: c["zs"][len(PLAN) - 1 - s], PLAN, eta, c["known"][which], dtype,
                                   variant, sd=sd64 if dtype == torch.float64 else sd32)
            out[eta, which] = dict(ref=run(torch.float64), f32=run(torch.float32), wrong={v: run(torch.float64, v) for v in VARIANTS})
    return c, out


# ---- known_level_table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_,taus", [(30, np.arange(30, dtype=np.int32)), (1000, ddim_timesteps(1000, 50))], ids=["identity30", "ddim50"])
def test_level_table_gathers_the_schedule_buffers(T_, taus):
    bufs = O.schedule_buffers("cosine", T_)
    sa, s1 = torch.sqrt(bufs["alphas_cumprod"]), torch.sqrt(1.0 - bufs["alphas_cumprod"])
    level = known_level_table(sa, s1, taus)
    assert level.dtype == np.float32 and level.shape == (len(taus), 2)
    assert level[0, 0] == np.float32(1.0) and level[0, 1] == np.float32(0.0)
    for s in range(1, len(taus)):
        assert level[s, 0].tobytes() == sa[int(taus[s - 1])].numpy().tobytes()
        assert level[s, 1].tobytes() == s1[int(taus[s - 1])].numpy().tobytes()
    assert np.array_equal(known_level_table(sa.numpy(), s1.numpy(), taus), level)


def test_level_table_rejects_a_timestep_outside_the_schedule():
    sa = np.linspace(1.0, 0.1, 30, dtype=np.float32)
    s1 = np.sqrt(1 - sa * sa)
    for bad in ([0, 30], [-1, 5], []):
        with pytest.raises(ValueError):
            known_level_table(sa, s1, np.array(bad, dtype=np.int32))


# ---- assemble_known -------------------------------------------------------------------------------------------------------------
def test_assemble_known():
    md, ed, pd_, n = 3, 5, 2, 4
    D = md + ed + pd_
    full = np.arange(n * D, dtype=np.float32).reshape(n, D)
    full[1, 4] = np.nan
    got = assemble_known(full, n, md, ed, pd_)
    assert got.dtype == np.float32 and got.shape == (n, D) and np.array_equal(got, full, equal_nan=True)
    assert np.array_equal(assemble_known(torch.from_numpy(full), n, md, ed, pd_), full, equal_nan=True)
    mut = np.array([[1, 0, 1]] * n, dtype=np.float64)
    expr = np.linspace(-1, 1, n * ed).reshape(n, ed)
    expr[2, 1] = np.nan
    path = np.ones((n, pd_))
    one = assemble_known({"mutations": mut}, n, md, ed, pd_)
    assert np.array_equal(one[:, :md], mut) and np.isnan(one[:, md:]).all()
    two = assemble_known({"mutations": mut, "pathways": path}, n, md, ed, pd_)
    assert np.array_equal(two[:, :md], mut) and np.isnan(two[:, md:md + ed]).all() and np.array_equal(two[:, md + ed:], path)
    three = assemble_known({"mutations": mut, "expression": expr, "pathways": path}, n, md, ed, pd_)
    assert np.array_equal(three[:, md:md + ed], expr.astype(np.float32), equal_nan=True) and np.isnan(three[2, md + 1])
    # one row broadcasts: an array, a block, a 1-D block
    row = assemble_known(full[:1], n, md, ed, pd_)
    assert row.shape == (n, D) and all(np.array_equal(row[i], full[0]) for i in range(n))
    b = assemble_known({"mutations": mut[:1], "pathways": torch.ones(pd_)}, n, md, ed, pd_)
    assert np.array_equal(b[:, :md], mut) and np.array_equal(b[:, md + ed:], path) and b.flags["C_CONTIGUOUS"]
    assert np.isnan(assemble_known({}, n, md, ed, pd_)).all()


@pytest.mark.parametrize("bad", [
    np.zeros((4, 9)),                                   # wrong width
    {"mutations": np.zeros((4, 4))},
    {"expression": np.zeros((4, 3))},
    np.zeros((3, 10)),                                  # neither 1 nor n rows
    {"pathways": np.zeros((2, 2))},
    np.full((4, 10), np.inf),                           # Inf
    {"mutations": np.array([[0.0, -np.inf, 1.0]])},
    {"genes": np.zeros((4, 3))},                        # no such block
], ids=["width", "width_mut", "width_expr", "rows", "rows_block", "inf", "inf_block", "key"])
def test_assemble_known_rejects(bad):
    with pytest.raises(ValueError):
        assemble_known(bad, 4, 3, 5, 2)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("eta", ETAS)
def test_restatement(chains, eta, which):
    """Known elements come back exactly; float32 agrees with float64 at the chain tolerance; each wrong chain does not."""
    c, out = chains
    r = out[eta, which]
    kn = c["known"][which]
    obs = ~torch.isnan(kn)
    assert 0 < obs.sum().item() < obs.numel()
    for name in ("ref", "f32"):
        assert torch.equal(r[name][obs].float(), kn[obs]), name
    ref = r["ref"]
    tol = tol_of(ref)
    err = (r["f32"].double() - ref).abs().max().item()
    print(f"eta={eta} {which}: max|ref|={ref.abs().max().item():.3e} tol={tol:.3e} fp32-fp64={err:.3e}")
    assert err <= tol
    for v, wrong in r["wrong"].items():
        d = (wrong - ref).abs().max().item()
        print(f"  {v}: {d:.3e} ({d / tol:.0f} x tol)")
        assert d > tol, v
