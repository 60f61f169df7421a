"""GPU: the strided DDIM sampler (ddim.py, osd_sample_chain_steps) on every reverse-chain engine -- the per-layer kernels with
and without hipGraph, the workspace, LDS-panel and squad (32 and 16 patients) chain kernels and the bf16x3 engine -- against a
float64 oracle that forms x^0, the direction term and sigma unfolded, and against each other."""
import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator
from osteosarcoma_diffusionmodel_amd.ddim import ddim_timesteps
from helpers import FULL, FULL_H, assert_close, block_widths, config, philox_keep_mask

pytestmark = pytest.mark.gpu

T, S, N = 100, 10, 300
RTOL, ATOL = 5e-5, 1e-5                   # the chain tests' tolerance: 5e-5 * max|ref| + 1e-5
ENGINES = {                               # (sampler, use_graph, chain_variant, squad_panel)
    "layers_graph": ("graph", True, None, None),
    "layers_eager": ("graph", False, None, None),
    "workspace": ("chain", True, "workspace", None),
    "panel": ("chain", True, "panel", None),
    "squad32": ("chain", True, "squad", 32),
    "squad16": ("chain", True, "squad", 16),
}


def _model(T_=T, seed=0, p=0.2, **dims):
    torch.manual_seed(seed)
    d = dict(FULL)
    d.update(dims)
    m = BiologyAwareDiffusionModel(config=config(FULL_H, T=T_, p=p), **d).cuda().eval()
    m.input_splitk = 0
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                  # non-trivial GroupNorm affine
        for k, prm in m.named_parameters():
            if k.endswith((".1.weight", ".5.weight")):
                prm.copy_((1 + 0.2 * torch.randn(prm.shape, generator=gen)).cuda())
            if k.endswith((".1.bias", ".5.bias")):
                prm.copy_((0.1 * torch.randn(prm.shape, generator=gen)).cuda())
    return m


def _use(m, engine):
    m.sampler, m.use_graph, m.chain_variant, m.squad_panel = ENGINES[engine]


def _run(m, engine, cond, n, **kw):
    _use(m, engine)
    out, mask = m.sample(cond, n, return_mutation_mask=True, **kw)
    sampler, _, variant, panel = ENGINES[engine]
    assert m.last_sampler == sampler, (engine, m.last_sampler)
    if sampler == "chain":
        assert m.last_chain_variant == variant, (engine, m.last_chain_variant)
    if panel:
        assert m.last_squad_panel == panel
    return out, mask


def _sd64(m):
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.startswith(("condition_embed", "unet"))}
    return O.to_dtype(sd, torch.float64)


def ddim_oracle(m, cond, x_T, zs, taus, eta, masks_fn=None, p=0.0):
    """The DDIM chain in float64, unfolded: x^0 = (x - sqrt(1-a) eps) / sqrt(a), x' = sqrt(a') x^0 + sqrt(1-a'-sigma^2) eps + sigma z,
    sigma = eta sqrt((1-a')/(1-a)) sqrt(1-a/a'), a' = 1 at the last step; z of step s is zs[S-1-s]."""
    sd = _sd64(m)
    Tm = m.num_steps
    abar = m.alphas_cumprod.detach().cpu().double()
    cond = cond.detach().cpu().double()
    x = x_T.detach().cpu().double()
    c_emb = O.condition_embed(sd, cond)
    n_s = len(taus)
    for s in reversed(range(n_s)):
        tau = int(taus[s])
        a = abar[tau]
        ap = abar[int(taus[s - 1])] if s > 0 else torch.tensor(1.0, dtype=torch.float64)
        t_norm = torch.full((x.shape[0],), tau / Tm, dtype=torch.float64)
        masks = masks_fn(s) if masks_fn is not None else None
        eps = O.unet_forward(sd, x, t_norm, c_emb, len(FULL_H), 128, masks, p)
        x0 = (x - torch.sqrt(1 - a) * eps) / torch.sqrt(a)
        sigma = eta * torch.sqrt((1 - ap) / (1 - a)) * torch.sqrt(1 - a / ap)
        x = torch.sqrt(ap) * x0 + torch.sqrt(torch.clamp(1 - ap - sigma ** 2, min=0.0)) * eps
        if s > 0 and zs is not None:
            x = x + sigma * zs[n_s - 1 - s].detach().cpu().double()
    return x


@pytest.fixture(scope="module")
def case():
    m = _model()
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(N, 3, generator=g)
    x_T = torch.randn(N, m.data_dim, generator=g)
    zs = torch.randn(S - 1, N, m.data_dim, generator=g)
    taus = ddim_timesteps(T, S)
    refs = {eta: ddim_oracle(m, cond, x_T, zs, taus, eta) for eta in (0.0, 0.5)}
    return m, cond.cuda(), x_T.cuda(), zs.cuda(), taus, refs


def _oracle_run(m, engine, case_, eta):
    _, cond, x_T, zs, _, _ = case_
    return _run(m, engine, cond, N, x_T=x_T, noise=zs if eta > 0 else None, seed=3, num_inference_steps=S, eta=eta)


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_against_fp64_oracle(case, engine, eta):
    m, *_, refs = case
    out, mask = _oracle_run(m, engine, case, eta)
    assert_close(out, refs[eta], RTOL, ATOL, f"{engine} eta={eta}")
    assert torch.equal(mask, (out[:, :m.mutation_dim] > 0.5).float())


def test_negative_controls(case):
    """The tolerance separates: timesteps moved down by one, or the other eta, land outside it."""
    m, cond, x_T, zs, taus, refs = case
    out, _ = _oracle_run(m, "layers_graph", case, 0.5)
    assert_close(out, refs[0.5], RTOL, ATOL, "control")
    tol = ATOL + RTOL * refs[0.5].abs().max().item()
    shifted = ddim_oracle(m, cond, x_T, zs, taus - 1, 0.5)
    assert (out.cpu().double() - shifted).abs().max().item() > tol
    assert (out.cpu().double() - refs[0.0]).abs().max().item() > tol


@pytest.fixture(scope="module")
def philox_case():
    m = _model(seed=2)
    cond = torch.randn(N, 3, generator=torch.Generator().manual_seed(5)).cuda()
    return m, cond


def test_engines_among_themselves(philox_case):
    m, cond = philox_case
    kw = dict(seed=77, row_offset=5, num_inference_steps=S, eta=0.5)
    ref, ref_mask = _run(m, "layers_graph", cond, N, **kw)
    out, mask = _run(m, "layers_eager", cond, N, **kw)
    assert torch.equal(out, ref) and torch.equal(mask, ref_mask)
    for engine in ("workspace", "panel"):
        out, mask = _run(m, engine, cond, N, **kw)
        assert torch.equal(out, ref) and torch.equal(mask, ref_mask), engine
        m.chain_steps_per_launch, m.chain_stagger = 3, 0
        out, mask = _run(m, engine, cond, N, **kw)
        m.chain_steps_per_launch, m.chain_stagger = 0, 30000          # the library's defaults
        assert torch.equal(out, ref) and torch.equal(mask, ref_mask), f"{engine}, segmented"
    for engine in ("squad32", "squad16"):
        out, _ = _run(m, engine, cond, N, **kw)
        assert_close(out, ref, 2e-5, 1e-6, engine)
        again, _ = _run(m, engine, cond, N, **kw)
        assert torch.equal(again, out), f"{engine} against itself"
    for steps in (1, T):
        kw1 = dict(kw, num_inference_steps=steps)
        ref1, ref1_mask = _run(m, "layers_graph", cond, N, **kw1)
        out1, mask1 = _run(m, "workspace", cond, N, **kw1)
        assert torch.isfinite(ref1).all()
        assert torch.equal(out1, ref1) and torch.equal(mask1, ref1_mask), f"S = {steps}"


def test_reduces_to_ddpm():
    """eta = 1 with every timestep is the DDPM chain: same x_T and the same Philox draws (step counter t), the coefficients
    agree to fp32 rounding of the two folds (test_ddim_cpu.py)."""
    m = _model(T_=30, seed=4)
    cond = torch.randn(N, 3, generator=torch.Generator().manual_seed(6)).cuda()
    _use(m, "layers_graph")
    ddpm = m.sample(cond, N, seed=9)
    ddim = m.sample(cond, N, seed=9, num_inference_steps=30, eta=1.0)
    assert_close(ddim, ddpm, RTOL, ATOL, "DDIM eta=1, S=T against DDPM")
    assert not torch.equal(ddim, m.sample(cond, N, seed=9, num_inference_steps=30, eta=0.0))


def test_bf16x3(case):
    m, *_, refs = case
    m.precision = "bf16x3"
    try:
        out, _ = _oracle_run(m, "layers_graph", case, 0.5)
        assert m.last_precision == "bf16x3"
    finally:
        m.precision = None
    assert_close(out, refs[0.5], RTOL, ATOL, "bf16x3")


@pytest.mark.parametrize("engine", list(ENGINES))
def test_no_leaked_state(philox_case, engine):
    m, cond = philox_case
    before, before_mask = _run(m, engine, cond, N, seed=21)
    _run(m, engine, cond, N, seed=22, num_inference_steps=7, eta=0.3)
    after, after_mask = _run(m, engine, cond, N, seed=21)
    assert torch.equal(before, after) and torch.equal(before_mask, after_mask)


def test_follows_the_parameters():
    """The plan's time-embedding rows are gathered per call from the current parameters: a DDIM call before and after an
    in-place update of time_proj.weight, the second against the oracle on the new weights."""
    m = _model(seed=7)
    g = torch.Generator().manual_seed(8)
    cond = torch.randn(N, 3, generator=g)
    x_T = torch.randn(N, m.data_dim, generator=g)
    taus = ddim_timesteps(T, S)
    for engine in ("layers_graph", "workspace"):
        _run(m, engine, cond.cuda(), N, x_T=x_T.cuda(), num_inference_steps=S)
        with torch.no_grad():
            m.unet.time_proj.weight.mul_(1.5)
        out, _ = _run(m, engine, cond.cuda(), N, x_T=x_T.cuda(), num_inference_steps=S)
        assert_close(out, ddim_oracle(m, cond, x_T, None, taus, 0.0), RTOL, ATOL, engine)


def test_real_dims_generate_scenarios():
    """The reference's dims (62 / 5054 / 26: D % 4 != 0, padded chain state) through generate_scenarios at S = 50: rows equal
    model.sample of the concatenated conditions, and the mask is (out[:, :62] > 0.5) of the same values."""
    m = _model(T_=1000, seed=3, mutation_dim=62, expression_dim=5054, pathway_dim=26)
    m.input_splitk = None
    gen = SyntheticPatientGenerator(m, config(FULL_H), device="cuda")
    scen = [{"name": f"s{k}", "conditions": {"survival_time": 300 + 400 * k, "event_occurred": k % 2, "metastasis_at_diagnosis": 1}}
            for k in range(3)]
    res = gen.generate_scenarios(scen, 333, seed=5, sampling_steps=50)
    cond = torch.cat([gen.create_conditions(333, sc["conditions"]) for sc in scen])
    out, mask = m.sample(cond, 999, seed=5, num_inference_steps=50, return_mutation_mask=True)
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    assert np.isfinite(out).all()
    for k, sc in enumerate(scen):
        r = slice(333 * k, 333 * (k + 1))
        got = res[sc["name"]]
        assert np.array_equal(got["expression"], out[r, 62:62 + 5054]) and np.array_equal(got["pathways"], out[r, 62 + 5054:])
        assert np.array_equal(got["mutations"], mask[r])
    assert np.array_equal(mask, (out[:, :62] > 0.5).astype(np.float32))


def test_sharding(philox_case):
    m, cond = philox_case
    kw = dict(seed=13, num_inference_steps=S, eta=1.0)
    whole, _ = _run(m, "layers_graph", cond, N, **kw)
    k = 128
    a, _ = _run(m, "layers_graph", cond[:k].contiguous(), k, row_offset=0, **kw)
    b, _ = _run(m, "layers_graph", cond[k:].contiguous(), N - k, row_offset=k, **kw)
    assert torch.equal(torch.cat([a, b]), whole)


def test_train_mode_dropout():
    """Train mode (dropout p = 0.2 inside the chain, per-layer kernels): keep masks of step s use Philox step counter s."""
    p, seed, n = 0.2, 41, 96
    m = _model(seed=9, p=p)
    g = torch.Generator().manual_seed(10)
    cond = torch.randn(n, 3, generator=g)
    x_T = torch.randn(n, m.data_dim, generator=g)
    zs = torch.randn(S - 1, n, m.data_dim, generator=g)
    m.train()
    try:
        _use(m, "layers_graph")
        out = m.sample(cond.cuda(), n, x_T=x_T.cuda(), noise=zs.cuda(), seed=seed, num_inference_steps=S, eta=0.5)
        assert m.last_sampler == "graph"
    finally:
        m.eval()
    widths = block_widths(FULL_H)

    def masks(s):
        return [torch.from_numpy(philox_keep_mask(seed, n, w, b, p, step=s)).double() for b, w in enumerate(widths)]

    ref = ddim_oracle(m, cond, x_T, zs, ddim_timesteps(T, S), 0.5, masks_fn=masks, p=p)
    assert_close(out, ref, RTOL, ATOL, "train mode")


def test_give_up_recovery():
    """A workspace chain that gives up in a dependency wait (one tile, two workgroups, spin budget of one tick) is re-run on the
    per-layer kernels with the same plan: the per-layer DDIM result, bit for bit."""
    n = 128
    m = _model(seed=6)
    g = torch.Generator().manual_seed(4)
    cond = torch.randn(n, 3, generator=g).cuda()
    x_T = torch.randn(n, m.data_dim, generator=g).cuda()
    kw = dict(x_T=x_T, seed=31, row_offset=7, num_inference_steps=S, eta=0.5)
    ref, ref_mask = _run(m, "layers_graph", cond, n, **kw)
    _use(m, "workspace")
    m.chain_grid, m.chain_spin_budget = 2, 1
    try:
        with pytest.warns(UserWarning, match="re-run on the per-layer kernels"):
            out, mask = m.sample(cond, n, return_mutation_mask=True, **kw)
    finally:
        m.chain_grid, m.chain_spin_budget = 0, 500_000_000
    assert m.last_sampler == "graph" and m.last_chain_variant == "workspace"
    assert torch.equal(out, ref) and torch.equal(mask, ref_mask)


def test_argument_errors(philox_case):
    m, cond = philox_case
    for kw in ({"num_inference_steps": 0}, {"num_inference_steps": T + 1}, {"num_inference_steps": S, "eta": 1.01},
               {"num_inference_steps": S, "eta": -0.1}, {"num_inference_steps": S, "noise": torch.zeros(S - 1, N, m.data_dim).cuda()}):
        with pytest.raises(ValueError):
            m.sample(cond, N, **kw)
    with pytest.raises(RuntimeError):
        m.sample(cond, N, num_inference_steps=S, eta=0.5, noise=torch.zeros(S, N, m.data_dim).cuda())
