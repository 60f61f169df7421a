"""GPU: the 128 x 128 instantiations of the posterior epilogue (EpiPosterior<MODE, KNOWN, LINK>, csrc/epilogues.h).  launch_posterior takes
the big tile from ceil(F/128) * ceil(P/128) >= 512 on; the known, clip, solver and link tests stay below that.  Here: the odd-dims model of
those tests (D = 5142, Dp = 5144: 41 feature tiles, the last partial) at n = 1600 rows (13 row tiles, the last of 64 rows: 533 tiles),
a plan of four steps on the per-layer engine, for each of plain, known, clip, clip + known, hist, hist + known, once with device Philox
draws on the padded state (the aligned kernels) and once with injected draws on the caller's rows (D % 4 = 2: the guarded kernels).

(a) 48 rows -- the first 16, 16 across the row-tile boundary at 128, the last 16 -- against the float64 restatements of the three
    files, fed those rows' own device draws (osd_op_randn), at those files' tolerance.  Rows are independent.
(b) the whole output and mask against the same request at sample_chunk_rows = 400 (41 x 4 = 164 tiles: the 64 x 128 tile), bit for bit.

LINK (osd_set_output_link): the same weights in a second model with prediction_type = "sample" and
mutation_link = "logistic" launch EpiPosterior<POST_CLIP | POST_HIST, KNOWN, true> -- clip_link, clip_known_link, hist_link,
hist_known_link -- on the same two operand paths of the big tile, where the bias is not prefetched (Pre is a dummy) and rides with the
x_t quads.  n_link = 62: of the four waves of a 128 x 128 tile (feature origins fw = 0 and 64 in the first feature tile) only fw = 0
takes the link walk, and the boundary lies mid-quad (62 = 60 + 2).  (a) is pred_helpers.chain64 / test_solver_cpu.dpmpp_chain with
link_helpers.link_out / link_eps_fn, the bounds and observations of the clip and known variants; (b) as above; and
test_gpu_link.check_link_block on the whole output.  The observations of these variants cover the whole mutation block, so
clip_known_link and hist_known_link show the link columns only through the history and the free columns beside them.

A third model with dims (200, 4916, 26) -- the same D, so the same tile counts -- repeats clip_known_link, hist_link and
hist_known_link: the link walk runs in the waves fw = 0, 64 of the first 128-wide feature tile and fw = 128, 192 of the second, and the
boundary lies inside the wave at 192 (200 = 192 + 8: a quad edge inside its 32-column block 0; blocks 1 of that wave select nothing).  There the mutation block of
the odd rows is left free, so that the KNOWN + LINK kernels write observed and linked elements side by side in the link columns.
"""
import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, _lib as L
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table
from helpers import FULL_H, assert_close, config
from link_helpers import link_eps_fn, link_out
from pred_helpers import chain64
from test_gpu_clip import chain_clipped, check_inside
from test_gpu_ddim import ddim_oracle
from test_gpu_known import chain_known, check_observed
from test_gpu_link import chain_link, chain_link_multistep, check_link_block
from test_gpu_solver import chain_multistep
from test_known_cpu import ATOL, PLAN, RTOL, T, known_chain, model_sd
from test_clip_cpu import clip_chain, mixed_bounds
from test_solver_cpu import dpmpp_chain

pytestmark = pytest.mark.gpu

DIMS, COND_DIM, N_ROWS, CHUNK = (62, 5054, 26), 3, 1600, 400
WIDE = (200, 4916, 26)                                    # the link past column 128, its boundary inside the wave at 192
D = sum(DIMS)
PLAN4 = PLAN[:4].copy()                                   # four steps, the last one the chain's step 0 (the mask store)
ETA = 0.5                                                 # plain, known, clip: a stochastic setting; the multistep solver has none
ROWS = np.r_[0:16, 120:136, N_ROWS - 16:N_ROWS]
SEED, OFF = (7 << 34) + 99, 11
VARIANTS = ("plain", "known", "clip", "clip_known", "hist", "hist_known")
LINK_VARIANTS = ("clip_link", "clip_known_link", "hist_link", "hist_known_link")
WIDE_VARIANTS = ("clip_known_link", "hist_link", "hist_known_link")


def chain_steps(m, cond, taus, eta, *, x_T=None, zs=None, seed=0, row_offset=0):
    """osd_sample_chain_steps through ctypes on the model's handle: (x_out, mutation mask)."""
    eng = m._engine()
    n = cond.shape[0]
    out = torch.empty(n, m.data_dim, device="cuda")
    mask = torch.empty(n, m.mutation_dim, device="cuda")
    tau, coef = ddim_step_table(m.alphas_cumprod, taus, eta)
    flags = L.OSD_F_GRAPH if m.use_graph else 0
    L.check(L.lib().osd_sample_chain_steps(eng.handle, L.ptr(cond), n, L.ptr(x_T), L.ptr(zs), seed, row_offset, L.ptr(out), L.ptr(mask), flags,
                                           tau.ctypes.data, coef.ctypes.data, int(tau.size)))
    torch.cuda.synchronize()
    return out, mask


def _case(dims, linked=False, free_odd_rows=False):
    """(model, inputs) of one model of ``dims``; the generator of the case.  free_odd_rows: the mutation block of the odd rows is not
    observed as a block (the 10 % scattered observations stay)."""
    assert sum(dims) == D
    assert D % 4 == 2 and ((D + 3) // 4 * 4 + 127) // 128 * ((N_ROWS + 127) // 128) >= 512 > (D + 127) // 128 * ((CHUNK + 127) // 128)
    md = dims[0]
    sd = O.init_state_dict(O.param_shapes(*dims, COND_DIM, FULL_H, 128), seed=33)
    conf = config(FULL_H, T=T)
    if linked:
        conf["model"]["diffusion"].update(prediction_type="sample", mutation_link="logistic")
    m = BiologyAwareDiffusionModel(*dims, COND_DIM, conf)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.input_splitk = 0
    m.sampler, m.use_graph = "graph", True
    g = torch.Generator().manual_seed(6)
    cond = torch.randn(N_ROWS, COND_DIM, generator=g)
    x0 = torch.randn(N_ROWS, D, generator=g)
    x0[:, :md] = (torch.rand(N_ROWS, md, generator=g) < 0.3).float()
    kn = torch.full((N_ROWS, D), float("nan"))
    kn[:, :md] = x0[:, :md]
    if free_odd_rows:
        kn[1::2, :md] = float("nan")
    pick = torch.rand(N_ROWS, D, generator=g) < 0.1
    kn[pick] = x0[pick]
    kn[:, D - 1] = x0[:, D - 1]                    # the last column, next to the pad
    lo, hi = mixed_bounds(*dims)
    lo[D - 2], hi[D - 2] = -0.5, 0.5               # bounds next to the pad
    eng = m._engine()

    def draws(step):                               # the device's own draws of the whole request: what the Philox runs generate
        a = torch.empty(N_ROWS, D, device="cuda")
        L.check(L.lib().osd_op_randn(eng.handle, L.ptr(a), N_ROWS, D, SEED, OFF, step, 0))
        return a

    x_T = draws(T)
    zs = {s: draws(s) for s in range(1, len(PLAN4))}
    c = dict(cond=cond.cuda(), kn=kn.cuda(), lo=lo, hi=hi, x_T=x_T, inj=torch.stack([zs[s] for s in range(len(PLAN4) - 1, 0, -1)]), md=md,
             sub=dict(cond=cond[ROWS], kn=kn[ROWS], x_T=x_T[ROWS].cpu(), zs={s: z[ROWS].cpu() for s, z in zs.items()}), sd64=model_sd(m, torch.float64))
    yield m, c
    m.sample_chunk_rows = 65536
    m._engine()
    m.sample_chunk_rows = None


@pytest.fixture(scope="module")
def case():
    yield from _case(DIMS)


@pytest.fixture(scope="module")
def link_case():
    yield from _case(DIMS, linked=True)


@pytest.fixture(scope="module")
def wide_case():
    yield from _case(WIDE, linked=True, free_odd_rows=True)


def run(m, c, variant, injected):
    draw = dict(x_T=c["x_T"], zs=c["inj"]) if injected else dict(seed=SEED, row_offset=OFF)
    kn = c["kn"] if "known" in variant else None
    if variant == "plain":
        return chain_steps(m, c["cond"], PLAN4, ETA, **draw)
    if variant == "known":
        return chain_known(m, c["cond"], kn, taus=PLAN4, eta=ETA, **draw)
    if variant.endswith("_link"):
        if variant.startswith("clip"):
            return chain_link(m, c["cond"], lo=c["lo"], hi=c["hi"], taus=PLAN4, eta=ETA, known=kn, **draw)
        return chain_link_multistep(m, c["cond"], c["lo"], c["hi"], PLAN4, known=kn, **draw)
    if variant.startswith("clip"):
        return chain_clipped(m, c["cond"], c["lo"], c["hi"], taus=PLAN4, eta=ETA, known=kn, **draw)
    return chain_multistep(m, c["cond"], c["lo"], c["hi"], PLAN4, known=kn, **draw)


def oracle(m, c, variant):
    s = c["sub"]
    kn = s["kn"] if "known" in variant else None
    if variant == "plain":
        return ddim_oracle(m, s["cond"], s["x_T"], [s["zs"][k] for k in range(len(PLAN4) - 1, 0, -1)], PLAN4, ETA)
    if variant == "known":
        return known_chain(m, s["cond"], s["x_T"], lambda k: s["zs"][k], PLAN4, ETA, kn, sd=c["sd64"])
    if variant.endswith("_link"):
        if variant.startswith("clip"):
            return chain64(m, s["cond"], s["x_T"], lambda k: s["zs"][k], PLAN4, ETA, "sample", sd=c["sd64"], out_fn=link_out(c["md"]), known=kn,
                           lo=c["lo"], hi=c["hi"])
        return dpmpp_chain(m, s["cond"], s["x_T"], lambda k: s["zs"][k], PLAN4, c["lo"], c["hi"], eps_fn=link_eps_fn(c["md"]), known=kn,
                           sd=c["sd64"], prediction="sample")
    if variant.startswith("clip"):
        return clip_chain(m, s["cond"], s["x_T"], lambda k: s["zs"][k], PLAN4, ETA, c["lo"], c["hi"], known=kn, sd=c["sd64"])
    return dpmpp_chain(m, s["cond"], s["x_T"], lambda k: s["zs"][k], PLAN4, c["lo"], c["hi"], known=kn, sd=c["sd64"])


def _both_tiles(m, c, variant):
    md = c["md"]
    ref = oracle(m, c, variant)
    obs = ~torch.isnan(c["kn"]) if "known" in variant else None
    linked = variant.endswith("_link")
    for injected in (False, True):
        tag = f"{variant} md={md} {'injected draws' if injected else 'padded state'}"
        m.sample_chunk_rows = 65536
        out, mask = run(m, c, variant, injected)
        assert L.lib().osd_sample_engine(m._engine().handle, -1, 0) == 0
        err = (out[ROWS].cpu().double() - ref).abs().max().item()
        print(f"{tag}: max|ref|={ref.abs().max().item():.3e} err={err:.3e}")
        assert_close(out[ROWS], ref, RTOL, ATOL, tag)                                     # (a)
        assert bool(torch.isfinite(out).all()) and torch.equal(mask, (out[:, :md] > 0.5).float())
        if obs is not None:
            check_observed(out, mask, c["kn"], md)
        if variant != "plain" and variant != "known":
            check_inside(out, mask, c["lo"], c["hi"], md, free=None if obs is None else ~obs)
        if linked:
            check_link_block(out, mask, md, free=None if obs is None else ~obs)
        m.sample_chunk_rows = CHUNK
        out_s, mask_s = run(m, c, variant, injected)
        print(f"{tag}: chunks of {CHUNK} rows differ by {(out_s - out).abs().max().item():.3e}")
        assert torch.equal(out_s, out) and torch.equal(mask_s, mask), tag                   # (b)


@pytest.mark.parametrize("variant", VARIANTS)
def test_big_tile_against_fp64_oracle_and_the_small_tile(case, variant):
    _both_tiles(*case, variant)


@pytest.mark.parametrize("variant", LINK_VARIANTS)
def test_big_tile_link_against_fp64_oracle_and_the_small_tile(link_case, variant):
    m, c = link_case
    assert m.mutation_link == "logistic" and c["md"] == 62
    _both_tiles(m, c, variant)


@pytest.mark.parametrize("variant", WIDE_VARIANTS)
def test_big_tile_link_past_column_128(wide_case, variant):
    m, c = wide_case
    md = c["md"]
    assert md == 200 and 128 < 192 < md < 192 + 32 and (md - 192) % 4 == 0          # two feature tiles; the boundary in block 0 of the wave at 192
    if "known" in variant:
        blk = ~torch.isnan(c["kn"][:, :md])
        assert bool(blk[0::2].all()) and bool((~blk[1::2]).any()) and bool(blk[1::2].any())
    _both_tiles(m, c, variant)
