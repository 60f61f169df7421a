"""GPU: the logistic link (osd_set_output_link) with its boundary past the first wave tile.  The link kernels
branch on a column position, each at its own granularity, and tests/test_gpu_link.py keeps n_link below 64 (62, 50, 16), where only the
wave at feature origin 0 ever takes the link code.  Both GEMM tiles give a wave 64 columns (two 32-column blocks, NFB = 2), so with
fw the wave's origin, fb its block and n_link = M:

    M       sampling: EpiPosterior<.., LINK>::apply, `fw < M` per wave      training: EpiLossT<true, true>::apply, `fw + 32 fb < M` per block
    32      wave 0 walks linked; its block 1 selects nothing                  block 0 linked, block 1 (origin 32 = M) is not
    64      wave 0 linked in every quad; the wave at 64 must NOT walk linked  blocks 0, 1 linked; the block at 64 is not
    98      waves 0, 64 linked; boundary mid-quad (98 = 96 + 2) in block 1    blocks 0 .. 96 linked, per-element select in the block at 96
    130     past the 128-wide tile: boundary mid-quad in the wave at 128      the block at 128 of the second workgroup tile selects
    200     (training only) 200 = 192 + 8: a quad edge inside the block at 192
    1950    nearly every column linked; boundary mid-quad (1948 + 2) in the ragged last tile (D = 2000 = 15 * 128 + 80)

Sampling (section 2 of the file).  D = 2000 (aligned: the LDS-DMA operand path of the 64 x 128 tile; 16 feature tiles x 1 row tile, far below
the 512 tiles of the big one), dims (M, 1974 - M, 26), 48 rows (one partial row tile), injected draws, the five-step PLAN of
tests/test_known_cpu.py at T = 100; and D = 5142 (D % 4 = 2), dims (98, 5018, 26) and (130, 4986, 26), 16 rows, twice with the same
draws (the device's own Philox draws, read back with osd_op_randn for the float64 chain):
    u98, u130    the device is handed the seed: the chain state lives in the padded buffer (Dp = 5144, F = ldx = Dp, fast_ok holds), so
                 these are the ALIGNED kernels with the pad columns next to the last feature tile
    g98, g130    the device is handed x_T and the draws as [16, 5142] arrays: the state stays on the caller's rows (ldx = 5142, rows not
                 16-byte aligned), fast_ok fails and the GUARDED vector kernels run -- the boundary mid-quad past column 64 (96 + 2)
                 and past the first workgroup tile (128 + 2) on that path
Modes: POST_CLIP at eta = 0.5 with infinite bounds;
POST_CLIP + KNOWN and POST_HIST + KNOWN with 30 % of the elements observed and bounds [0.45, 0.55] that cut into the link's range.
Every point: the float64 chain (pred_helpers.chain64 / test_solver_cpu.dpmpp_chain with link_helpers.link_out / link_eps_fn) at
tol_of = 5e-5 max|ref| + 1e-5; test_gpu_link.check_link_block; and two controls -- against the chain that links M + 2 columns the
columns [M, M + 2) miss the tolerance, against the one that links M - 2 the columns [M - 2, M) do.  A control is used only after the
two float64 chains were seen to differ on those columns by more than twice the tolerance (the device is within one of the first, so
it is more than one away from the second).

Training (section 1).  EpiLossT<true, true> on its three operand paths, hidden [256, 512, 256]:
    guard16    D = 5142, dims (M, 5116 - M, 26, 4), 16 rows, injected masks: D % 4 = 2, the guarded epilogue of the 64 x 128 tile
    xpose37    D = 2000, dims (M, 1950 - M, 50, 3), 37 rows: the transposer path (f and fo differ); (1950, 24, 26, 3) for M = 1950
    big2111    D = 2000, 2111 rows: ceil(2000/128) * ceil(2111/128) = 16 * 17 = 272 >= 256 tiles, the 128 x 128 tile (launch.h:
               use_big_tile), transposer path, ragged last row tile (2111 = 16 * 128 + 63)
against link_helpers.LinkOracle: loss_helpers.check (loss 1e-5 relative; every gradient tensor 5e-5 of its own max), and
link_helpers.check_boundary: output_proj's bias gradient and weight-gradient rows at B = [M - 8, M + 8) + {31, 32, 63, 64, 127, 128},
element by element, against GRAD_RTOL * max|ref on B| + 1e-9 -- relative to the boundary columns, not to a 2000-row tensor.  The
reference's own fp32 noise fits that bound: a torch fp32 restatement of the same loss (link_helpers.fp32_link_grads) errs by less than
0.03 of it over the 22 small-group cases on the hosts it was run on (the figure moves with the host's BLAS code path and thread count;
test_link_cpu.py: test_fp32_restatement_fits_the_boundary_bound holds every one of them below 0.1), so the bound stands unwidened.
Controls (small groups): the oracle with M + 1 and the one with M - 1 link columns each fail check_boundary, after the two float64
oracles were seen to differ on B by more than twice the bound.

Saturated logits (section 3), xpose37 / the D = 2000 sampling model at M = 98: output_proj's bias at the link columns 0, 31, 64, 97
is +100, -100, +40, -40.  exp2 overflows to +inf (rcp -> 0) or flushes to 0 there; a 0 * inf or a flushed denormal in the wrong place
would be a NaN loss or a value outside [0, 1].
"""
import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
from osteosarcoma_diffusionmodel_amd import _lib as L
from osteosarcoma_diffusionmodel_amd.train import _loss_fwd_bwd
from helpers import FULL_H, config
from link_helpers import (SAT_BIAS, SAT_COLS, TILE_GROUPS, TILE_OBJECTIVES, boundary_columns, check_boundary, link_eps_fn, link_out,
                          tile_dims, tile_reference, tile_shape)
from loss_helpers import GRAD_RTOL, LOSS_RTOL, P_DROP, SEED, check
from mask_helpers import H3
from pred_helpers import chain64
from test_clip_cpu import mixed_bounds
from test_gpu_ddim import _use
from test_gpu_link import LINK, LOSS_EPI, MASKED, _option, chain_link, chain_link_multistep, check_link_block
from test_known_cpu import PLAN, T, model_sd, tol_of
from test_solver_cpu import dpmpp_chain

pytestmark = pytest.mark.gpu

_cache = {}


# ======== 1. training: EpiLossT<true, true> =============================================================================================
GROUPS, OBJECTIVES, train_dims, _shape, _reference = TILE_GROUPS, TILE_OBJECTIVES, tile_dims, tile_shape, tile_reference      # link_helpers.py
SMALL = [(g, M) for g in ("guard16", "xpose37") for M in GROUPS[g]["Ms"]]
TRAIN_CASES = [(g, M, obj) for g, M in SMALL for obj in ("l2", "huber0.3-minsnr-masked")] + [("big2111", M, "l2-masked") for M in GROUPS["big2111"]["Ms"]]


def _device(group, M, obj, sat=False):
    """(loss, {name: gradient}, last_train_path, output_link) of one training call on the device (cached)."""
    key = ("dev", group, M, obj, sat)
    if key not in _cache:
        kind, delta, weighting, masked = OBJECTIVES[obj]
        g = GROUPS[group]
        mut, expr, pw, cd = train_dims(group, M)
        sd, x, cond, t, noise, injected, _ = _shape(group, M, masked, sat)
        conf = config(H3, p=P_DROP)
        conf["model"]["diffusion"].update(prediction_type="sample", mutation_link="logistic", loss_type=kind, huber_delta=delta,
                                          loss_weighting="min_snr" if weighting == "min_snr" else None)
        if masked:
            conf["training"] = {"missing_values": "mask"}
        m = BiologyAwareDiffusionModel(config=conf, mutation_dim=mut, expression_dim=expr, pathway_dim=pw, condition_dim=cd)
        m.load_state_dict(sd, strict=False)
        m = m.cuda().train()
        grads = [torch.empty_like(p) for p in m.parameters()]
        kw = dict(t=t.cuda(), noise=noise.cuda(), seed=SEED)
        if g["draw"] == "injected":
            kw["dropout_masks"] = [k.cuda() for k in injected]
        loss = _loss_fwd_bwd(m, x.cuda(), cond.cuda(), L.ptr_array(grads), **kw)
        torch.cuda.synchronize()
        names = [k for k, _ in m.named_parameters()]
        _cache[key] = (loss.item(), {k: v.cpu() for k, v in zip(names, grads)}, _option(m, b"last_train_path"), _option(m, b"output_link"))
    return _cache[key]


def _hold(group, M, obj, sat=False, extra=()):
    kind, delta, weighting, masked = OBJECTIVES[obj]
    D = GROUPS[group]["D"]
    tag = f"{group} M={M} {obj}{' saturated' if sat else ''}"
    got, ref = _device(group, M, obj, sat), _reference(group, M, obj, sat)
    worst, bad = check(got[0], got[1], ref[0], ref[1], D, show=tag)
    print(f"[{tag}] loss {got[0]:.8g} (fp64 {ref[0]:.8g}); worst error / tolerance {worst:.3f}")
    assert not bad, "\n".join(bad)
    worst_b, bad_b = check_boundary(got[1], ref[1], boundary_columns(M, D, extra), GRAD_RTOL, show=tag)
    assert not bad_b, "\n".join(bad_b)
    path = got[2]
    assert path & LINK and path & LOSS_EPI, f"last_train_path {path:#x}: the link epilogue did not run"
    assert bool(path & MASKED) == masked, f"last_train_path {path:#x}"
    assert got[3] == M
    return got, ref


@pytest.mark.parametrize("group,M,obj", TRAIN_CASES, ids=[f"{g}-{M}-{o}" for g, M, o in TRAIN_CASES])
def test_link_boundary_training_vs_fp64(group, M, obj):
    g = GROUPS[group]
    big = (g["D"] + 127) // 128 * ((g["n"] + 127) // 128)
    if group == "big2111":
        assert (g["D"] + 127) // 128 == 16 and (g["n"] + 127) // 128 == 17 and big == 272 >= 256
    else:
        assert big < 256
    assert (g["D"] % 4 == 2) == (group == "guard16")
    _hold(group, M, obj)


@pytest.mark.parametrize("group,M", SMALL, ids=[f"{g}-{M}" for g, M in SMALL])
def test_link_boundary_training_controls(group, M):
    """One link column too many or too few fails the boundary-column check (and the device passes it against the right oracle)."""
    obj, D = "l2", GROUPS[group]["D"]
    got, ref = _device(group, M, obj), _reference(group, M, obj)
    cols = boundary_columns(M, D)
    idx = torch.as_tensor(cols)
    assert not check_boundary(got[1], ref[1], cols, GRAD_RTOL)[1]
    for other in (M + 1, M - 1):
        ctl = _reference(group, M, obj, link=other)
        apart = 0.0
        for key in ("unet.output_proj.bias", "unet.output_proj.weight"):
            bound = GRAD_RTOL * ref[1][key][idx].abs().max().item() + 1e-9
            apart = max(apart, (ctl[1][key][idx] - ref[1][key][idx]).abs().max().item() / bound)
        print(f"[{group} M={M}] the oracle with {other} link columns is {apart:.1f} bounds away on the boundary columns")
        assert apart > 2.0, "the control checks nothing: the two float64 oracles agree on the boundary columns"
        assert check_boundary(got[1], ctl[1], cols, GRAD_RTOL, show=f"{group} M={M} control {other}")[1], f"{other} link columns went unnoticed"


def test_saturated_logits_training():
    group, M, obj = "xpose37", 98, "l2"
    orc = _shape(group, M, False, True)[6]
    pred = orc.pred.detach()
    assert float(pred[:, [0, 31]].abs().min()) > 90 and float(pred[:, [64, 97]].abs().min()) > 30
    got, ref = _hold(group, M, obj, sat=True, extra=SAT_COLS)
    assert np.isfinite(got[0]) and all(bool(torch.isfinite(v).all()) for v in got[1].values())
    # a confident wrong call costs |o| ~ 100 where an element of the other columns costs ~ 1: the four columns' share of the loss is
    # thousands of loss tolerances, so the loss comparison above sees them
    n, D = pred.shape
    y = orc.inner.x0[:, list(SAT_COLS)]
    rho = torch.nn.functional.binary_cross_entropy_with_logits(pred[:, list(SAT_COLS)], y, reduction="none")
    share = rho.sum().item() / (n * D)
    print(f"saturated columns: {share:.6g} of the loss {ref[0]:.6g}; the largest element {rho.max().item():.4g}")
    assert rho.max().item() > 90 and share > 1000 * LOSS_RTOL * ref[0]


# ======== 2. sampling: EpiPosterior<POST_CLIP | POST_HIST, KNOWN, true> on the 64 x 128 tile =============================================
SWEEP = {M: (M, 1974 - M, 26) for M in (32, 64, 98, 130, 1950)}                  # D = 2000: 48 rows, injected draws
SWEEP.update({f"u{M}": (M, 5116 - M, 26) for M in (98, 130)})                      # D = 5142: 16 rows, device draws on the padded state
SWEEP.update({f"g{M}": (M, 5116 - M, 26) for M in (98, 130)})                      # ... and the same draws injected on the caller's rows
MODES = ("clip", "known_clip", "known_hist")
ETA = 0.5
PHILOX = ((7 << 34) + 99, 11)


def sample_model(dims, sat=False):
    """A linked "sample" model of ``dims`` on the per-layer engine (tests/test_gpu_link.py: test_unaligned_dims_on_the_padded_state)."""
    sd = O.init_state_dict(O.param_shapes(*dims, 3, FULL_H, 128), seed=33)
    if sat:
        sd["unet.output_proj.bias"][list(SAT_COLS)] = torch.tensor(SAT_BIAS)
    conf = config(FULL_H, T=T)
    conf["model"]["diffusion"].update(prediction_type="sample", mutation_link="logistic")
    m = BiologyAwareDiffusionModel(*dims, 3, conf)
    m.load_state_dict(sd, strict=False)
    return m.eval()


def sample_inputs(m, n, draws=None):
    """Conditions, the start, one draw per step (z[s], s = 1 .. S - 1), 30 % observations and the bounds of the known modes.
    draws(step) -> [n, D]: the device's own Philox draws (the start is then pure noise); None: host draws and a noised patient."""
    M, D, S = m.mutation_dim, m.data_dim, len(PLAN)
    g = torch.Generator().manual_seed(11)
    cond = torch.randn(n, 3, generator=g)
    x0 = torch.randn(n, D, generator=g)
    x0[:, :M] = (torch.rand(n, M, generator=g) < 0.3).float()
    if draws is None:
        a = m.alphas_cumprod.detach().cpu()[int(PLAN[-1])]
        x_start = torch.sqrt(a) * x0 + torch.sqrt(1 - a) * torch.randn(n, D, generator=g)
        z = {s: torch.randn(n, D, generator=g) for s in range(1, S)}
    else:
        x_start, z = draws(T), {s: draws(s) for s in range(1, S)}
    kn = torch.full_like(x0, float("nan"))
    pick = torch.rand(x0.shape, generator=torch.Generator().manual_seed(31)) < 0.3
    kn[pick] = x0[pick]
    lo, hi = mixed_bounds(M, m.expression_dim, m.pathway_dim)
    lo[:M], hi[:M] = 0.45, 0.55                      # the clamp cuts into the link's range
    return dict(cond=cond, x_start=x_start, z=z, kn=kn, lo=lo, hi=hi)


def chain_ref(m, c, mode, n_link, sd64):
    """The float64 chain of ``mode`` with the link on the columns [0, n_link)."""
    z_of_s = lambda s: c["z"][s]
    if mode == "clip":
        return chain64(m, c["cond"], c["x_start"], z_of_s, PLAN, ETA, "sample", sd=sd64, out_fn=link_out(n_link))
    if mode == "known_clip":
        return chain64(m, c["cond"], c["x_start"], z_of_s, PLAN, ETA, "sample", sd=sd64, out_fn=link_out(n_link), known=c["kn"], lo=c["lo"], hi=c["hi"])
    if mode == "known_hist":
        return dpmpp_chain(m, c["cond"], c["x_start"], z_of_s, PLAN, c["lo"], c["hi"], eps_fn=link_eps_fn(n_link), known=c["kn"], sd=sd64,
                           prediction="sample")
    assert mode == "hist"
    return dpmpp_chain(m, c["cond"], c["x_start"], None, PLAN, None, None, eps_fn=link_eps_fn(n_link), sd=sd64, prediction="sample")


def controls_apart(ref, wider, narrower, M):
    """The float64 chains that link M + 2 and M - 2 columns, in tolerances, on the columns where they differ from the chain of M."""
    tol = tol_of(ref)
    return (wider - ref)[:, M:M + 2].abs().max().item() / tol, (narrower - ref)[:, M - 2:M].abs().max().item() / tol


def chain_dev(m, c, mode, draw):
    cond = c["cond"].cuda()
    if mode == "clip":
        return chain_link(m, cond, taus=PLAN, eta=ETA, **draw)
    if mode == "known_clip":
        return chain_link(m, cond, lo=c["lo"], hi=c["hi"], taus=PLAN, eta=ETA, known=c["kn"].cuda(), **draw)
    if mode == "known_hist":
        return chain_link_multistep(m, cond, c["lo"], c["hi"], PLAN, known=c["kn"].cuda(), **draw)
    draw = {k: v for k, v in draw.items() if k != "zs"}              # the solver takes draws only for observed elements
    return chain_link_multistep(m, cond, None, None, PLAN, **draw)


def _sweep_case(key, sat=False):
    """(model on the device, inputs, how the device gets its draws, fp64 weights) of one sweep point (cached).  The u and g points of one
    M share the model, the inputs and the draws: u hands the device the seed (the padded state), g the draws themselves."""
    dims = SWEEP[key]
    ck = ("sweep", dims, sat)
    if ck not in _cache:
        D = sum(dims)
        m = sample_model(dims, sat).cuda()
        m.input_splitk = 0
        _use(m, "layers_graph")
        if D % 4 == 0:
            c = sample_inputs(m, 48)
        else:
            assert D % 4 == 2
            n, eng = 16, m._engine()

            def draws(step):                       # the device's own draws of the request: what the Philox run generates
                a = torch.empty(n, D, device="cuda")
                L.check(L.lib().osd_op_randn(eng.handle, L.ptr(a), n, D, PHILOX[0], PHILOX[1], step, 0))
                return a.cpu()
            c = sample_inputs(m, n, draws)
        _cache[ck] = (m, c, model_sd(m, torch.float64))
    m, c, sd64 = _cache[ck]
    if str(key).startswith("u"):
        draw = dict(seed=PHILOX[0], row_offset=PHILOX[1])
    else:                                          # [n, D] arrays of the caller: at D % 4 = 2 their rows are not 16-byte aligned
        draw = dict(x_T=c["x_start"].cuda(), zs=torch.stack([c["z"][s] for s in range(len(PLAN) - 1, 0, -1)]).cuda())
    return m, c, draw, sd64


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", list(SWEEP))
def test_link_boundary_sampling_vs_fp64(key, mode):
    m, c, draw, sd64 = _sweep_case(key)
    M, D = m.mutation_dim, m.data_dim
    assert (D + 127) // 128 * ((c["cond"].shape[0] + 127) // 128) < 512                  # the 64 x 128 tile
    out, mask = chain_dev(m, c, mode, draw)
    assert L.lib().osd_sample_engine(m._engine().handle, -1, 0) == 0
    ref = chain_ref(m, c, mode, M, sd64)
    tol = tol_of(ref)
    got = out.cpu().double()
    err = (got - ref).abs().max().item()
    print(f"[{key} {mode}] max|ref|={ref.abs().max().item():.3e} tol={tol:.3e} err={err:.3e}")
    assert err <= tol
    obs = None
    if mode != "clip":
        obs = ~torch.isnan(c["kn"]).cuda()
        assert torch.equal(out[obs], c["kn"].cuda()[obs])
        free = ~obs[:, :M]
        lo_t, hi_t = torch.from_numpy(c["lo"][:M]).cuda(), torch.from_numpy(c["hi"][:M]).cuda()
        assert bool((((out[:, :M] >= lo_t) & (out[:, :M] <= hi_t)) | ~free).all())
    check_link_block(out, mask, M, free=None if obs is None else ~obs)
    # the controls: two link columns too many, two too few
    wider, narrower = chain_ref(m, c, mode, M + 2, sd64), chain_ref(m, c, mode, M - 2, sd64)
    up, down = controls_apart(ref, wider, narrower, M)
    print(f"[{key} {mode}] fp64 chains with M + 2 / M - 2 link columns: {up:.1f} / {down:.1f} tolerances away")
    assert up > 2.0 and down > 2.0, "a control checks nothing: the float64 chains agree on its columns"
    assert (got - wider)[:, M:M + 2].abs().max().item() > tol, "two link columns too many went unnoticed"
    assert (got - narrower)[:, M - 2:M].abs().max().item() > tol, "two link columns too few went unnoticed"


# ======== 3. saturated logits in the sampling step ========================================================================================
@pytest.mark.parametrize("mode", ["clip", "hist"])
def test_saturated_logits_sampling(mode):
    m, c, draw, sd64 = _sweep_case(98, sat=True)
    M = m.mutation_dim
    out, mask = chain_dev(m, c, mode, draw)
    ref = chain_ref(m, c, mode, M, sd64)
    tol = tol_of(ref)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"[saturated {mode}] max|ref|={ref.abs().max().item():.3e} tol={tol:.3e} err={err:.3e}; columns {SAT_COLS}: "
          f"{[(out[:, k].min().item(), out[:, k].max().item()) for k in SAT_COLS]}")
    assert bool(torch.isfinite(out).all())
    assert bool((out[:, 0] == 1.0).all()) and bool((out[:, 31] == 0.0).all())          # |bias| = 100: exactly 1 and 0
    assert bool(((out[:, [64, 97]] >= 0) & (out[:, [64, 97]] <= 1)).all())
    assert float(out[:, 64].min()) > 0.5 > float(out[:, 97].max())
    check_link_block(out, mask, M)
    assert err <= tol
