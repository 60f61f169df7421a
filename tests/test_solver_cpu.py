"""Host: the DPM-Solver++(2M) multistep sampler -- its step table (ddim.dpmpp_2m_table), the log-SNR step spacing
(ddim.logsnr_timesteps), a CPU restatement of the chain in float64 and float32, the solver's accuracy on a Gaussian toy whose
probability-flow solution is known in closed form, and the controls that show the chain tolerance separates a chain without history, one
whose history is the unclipped x0 and one whose history is a step too old.  tests/test_gpu_solver.py holds the device to the same float64
restatement."""
import math

import numpy as np
import pytest
import torch

from oracle import diffusion_oracle as O
from osteosarcoma_diffusionmodel_amd.ddim import (ddim_step_table, ddim_timesteps, ddim_x0_table, dpmpp_2m_table, known_level_table,
                                                 logsnr_timesteps)
from helpers import FULL_H
from test_known_cpu import N, PLAN, T, cpu_model, make_case, model_sd, tol_of
from test_clip_cpu import clip_chain, mixed_bounds

VARIANTS = ("no_history", "raw_history", "stale_history")
PREDICTIONS = ("epsilon", "v_prediction", "sample")


def dpmpp_chain(m, cond, x_start, z_of_s, taus, lo, hi, dtype=torch.float64, variant=None, eps_fn=None, known=None, *, sd=None,
                prediction="epsilon"):
    """The DPM-Solver++(2M) chain on the CPU.  Step s goes from tau_s to tau' = tau_{s-1}, s = S-1 first; with alpha = sqrt(abar),
    sigma = sqrt(1-abar), lambda = ln(alpha/sigma), h = lambda' - lambda, phi = alpha' (1 - exp(-h)):
        x0  = (x - sigma out)/alpha   (epsilon; v_prediction: a x - b out with the model's buffers; sample: out),   x0c = clamp(x0, lo, hi)
        D   = x0c                                         the first step run, and every step when S <= 2
        D   = (1 + 1/(2r)) x0c - 1/(2r) x0c_prev          r = (lambda_s - lambda_{s+1})/h, otherwise
        x'  = (sigma'/sigma) x + phi D;                   x' = x0c at s = 0
    float64: these expressions in double from the fp32 alphas_cumprod buffer.  float32: the tables the library is handed
    (dpmpp_2m_table) in the library's operation order.  lo = hi = None: unbounded.
    variant: one of VARIANTS -- a deliberately wrong chain.  eps_fn(sd, x, t_norm, cond): another denoiser evaluation (guidance).
    known: observed elements (NaN = free) are put back after every step as tests/test_known_cpu.known_chain does, with the draw
    z_of_s(s); the history keeps the clipped network prediction."""
    sd = model_sd(m, dtype) if sd is None else sd
    cond = cond.detach().cpu().to(dtype)
    x = x_start.detach().cpu().to(dtype)
    taus = np.asarray(taus)
    n_s = len(taus)
    lo_t = None if lo is None else torch.as_tensor(lo).to(dtype)
    hi_t = None if hi is None else torch.as_tensor(hi).to(dtype)
    abar = m.alphas_cumprod.detach().cpu().double()
    sa_buf, s1_buf = m.sqrt_alphas_cumprod.detach().cpu().double(), m.sqrt_one_minus_alphas_cumprod.detach().cpu().double()
    if dtype == torch.float32:
        _, tab, hist_tab = dpmpp_2m_table(m.alphas_cumprod, taus, prediction, sqrt_alphas_cumprod=m.sqrt_alphas_cumprod,
                                          sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod)
        tab, hist_tab = torch.from_numpy(tab), torch.from_numpy(hist_tab)
        level = torch.from_numpy(known_level_table(m.sqrt_alphas_cumprod, m.sqrt_one_minus_alphas_cumprod, taus))
    kn = obs = None
    if known is not None:
        kn = known.detach().cpu().to(dtype)
        obs = ~torch.isnan(kn)
    c_emb = O.condition_embed(sd, cond)
    lam = 0.5 * (torch.log(abar) - torch.log1p(-abar))

    def clamp(v):
        return v if lo_t is None else torch.minimum(torch.maximum(v, lo_t), hi_t)

    older = prev = None                  # the history: x0c of step s + 2 and of step s + 1
    for s in reversed(range(n_s)):
        tau = int(taus[s])
        t_norm = torch.full((x.shape[0],), tau / m.num_steps, dtype=dtype)
        out = O.unet_forward(sd, x, t_norm, c_emb, len(FULL_H), 128, None, 0.0) if eps_fn is None else eps_fn(sd, x, t_norm, cond)
        z = z_of_s(s).detach().cpu().to(dtype) if (s > 0 and kn is not None) else None
        second_order = 0 < s < n_s - 1 and n_s > 2
        if dtype == torch.float32:
            P, Q, G, F = tab[s]
            x0 = P * x + Q * out
            x0c = clamp(x0)
            h_prev = prev if (second_order and float(hist_tab[s]) != 0.0) else torch.zeros_like(x)
            nxt = G * x0c + (F * x + hist_tab[s] * h_prev)
        else:
            a = abar[tau]
            if prediction == "epsilon":
                x0 = (x - torch.sqrt(1 - a) * out) / torch.sqrt(a)
            elif prediction == "v_prediction":
                x0 = sa_buf[tau] * x - s1_buf[tau] * out
            else:
                x0 = out
            x0c = clamp(x0)
            if s == 0:
                nxt = x0c
            else:
                tp = int(taus[s - 1])
                ap = abar[tp]
                h = lam[tp] - lam[tau]
                phi = -torch.sqrt(ap) * torch.expm1(-h)
                d = x0c
                if second_order:
                    r = (lam[tau] - lam[int(taus[s + 1])]) / h
                    used = older if (variant == "stale_history" and older is not None) else prev
                    if variant != "no_history":
                        d = (1 + 1 / (2 * r)) * x0c - used / (2 * r)
                nxt = torch.sqrt(1 - ap) / torch.sqrt(1 - a) * x + phi * d
        older, prev = prev, (x0 if variant == "raw_history" else x0c)
        x = nxt
        if kn is not None:
            if s == 0:
                x = torch.where(obs, kn, x)
            elif dtype == torch.float32:
                x = torch.where(obs, level[s, 0] * kn + level[s, 1] * z, x)
            else:
                ap = abar[int(taus[s - 1])]
                x = torch.where(obs, torch.sqrt(ap) * kn + torch.sqrt(1 - ap) * z, x)
    return x


def cosine_abar(T_=1000):
    return O.schedule_buffers("cosine", T_)["alphas_cumprod"]


# ---- dpmpp_2m_table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
@pytest.mark.parametrize("S", [3, 10, 50])
def test_table_rows(S, spacing):
    abar = cosine_abar()
    taus = ddim_timesteps(1000, S) if spacing == "uniform" else logsnr_timesteps(abar, S)
    tau, tab, hist = dpmpp_2m_table(abar, taus)
    assert tau.dtype == np.int32 and np.array_equal(tau, taus)
    assert tab.dtype == np.float32 and tab.shape == (S, 4) and hist.dtype == np.float32 and hist.shape == (S,)
    assert np.isfinite(tab).all() and np.isfinite(hist).all()
    # row 0 and row S-1, exactly
    assert tab[0, 2] == np.float32(1.0) and tab[0, 3] == np.float32(0.0) and hist[0] == np.float32(0.0)
    a64 = abar.numpy().astype(np.float64)
    al, si = np.sqrt(a64[taus]), np.sqrt(1.0 - a64[taus])
    lam = np.log(al / si)
    phi_first = -al[S - 2] * math.expm1(-(lam[S - 2] - lam[S - 1]))
    assert hist[S - 1] == np.float32(0.0)
    assert tab[S - 1, 2] == np.float32(phi_first) and tab[S - 1, 3] == np.float32(si[S - 2] / si[S - 1])
    # H < 0 < G on interior rows
    assert (hist[1:S - 1] < 0).all() and (tab[1:S - 1, 2] > 0).all()
    # G + H and F are DDIM's E and F at eta = 0.  Every entry is the fp32 rounding of a float64 value: half a spacing each, and the
    # float64 values behind G + H and behind E differ by a few float64 roundings of |G| + |H| (2r ~ 2, so |G|, |H| stay of E's order)
    ref = ddim_x0_table(abar, taus, 0.0)
    G, F, H = tab[:, 2].astype(np.float64), tab[:, 3].astype(np.float64), hist.astype(np.float64)
    E = ref[:, 2].astype(np.float64)
    tol_e = 0.5 * (np.spacing(tab[:, 2]) + np.spacing(np.abs(hist)) + np.spacing(np.abs(ref[:, 2]))) + 64 * np.finfo(np.float64).eps * (np.abs(G) + np.abs(H))
    assert (np.abs(G + H - E) <= tol_e).all(), np.abs(G + H - E).max()
    tol_f = 0.5 * (np.spacing(tab[:, 3]) + np.spacing(ref[:, 3])) + 64 * np.finfo(np.float64).eps * np.abs(F)
    assert (np.abs(F - ref[:, 3].astype(np.float64)) <= tol_f).all()
    # a numpy buffer gives the same table
    t2 = dpmpp_2m_table(abar.numpy(), taus)
    assert np.array_equal(t2[1], tab) and np.array_equal(t2[2], hist)


@pytest.mark.parametrize("S", [1, 2])
def test_one_and_two_steps_are_ddim(S):
    abar = cosine_abar()
    taus = ddim_timesteps(1000, S)
    _, tab, hist = dpmpp_2m_table(abar, taus)
    assert (hist == 0).all()
    ref = ddim_x0_table(abar, taus, 0.0)
    assert np.array_equal(tab[:, :2], ref[:, :2])
    assert np.abs(tab[:, 2:].astype(np.float64) - ref[:, 2:]).max() <= np.spacing(np.abs(ref[:, 2:])).max()
    # ... and so is the chain: the restatement against test_clip_cpu's DDIM chain at eta = 0
    m = cpu_model()
    c = make_case(m)
    lo, hi = mixed_bounds()
    plan = PLAN[-S:]
    sd64 = model_sd(m, torch.float64)
    got = dpmpp_chain(m, c["cond"], c["x_start"], lambda s: None, plan, lo, hi, sd=sd64)
    ref_chain = clip_chain(m, c["cond"], c["x_start"], lambda s: torch.zeros_like(c["x_start"]), plan, 0.0, lo, hi, sd=sd64)
    assert (got - ref_chain).abs().max().item() <= 1e-12 * max(1.0, ref_chain.abs().max().item())


@pytest.mark.parametrize("prediction", PREDICTIONS)
def test_table_reads_x0_as_the_ddim_table_does(prediction):
    abar = cosine_abar()
    taus = ddim_timesteps(1000, 20)
    sched = dict(sqrt_alphas_cumprod=torch.sqrt(abar), sqrt_one_minus_alphas_cumprod=torch.sqrt(1.0 - abar))
    _, tab, hist = dpmpp_2m_table(abar, taus, prediction, **sched)
    ref = ddim_x0_table(abar, taus, 0.0, prediction, **sched)
    assert np.array_equal(tab[:, :2], ref[:, :2])
    _, eps_tab, eps_hist = dpmpp_2m_table(abar, taus)
    assert np.array_equal(tab[:, 2:], eps_tab[:, 2:]) and np.array_equal(hist, eps_hist)      # only (P, Q) depend on the type


def test_table_rejects():
    abar = np.linspace(0.99, 0.01, 30, dtype=np.float32)
    for bad in ([0, 30], [-1, 5], []):
        with pytest.raises(ValueError):
            dpmpp_2m_table(abar, np.array(bad, dtype=np.int32))
    for bad in ([5, 5, 9], [3, 9, 7], [9, 5, 2]):            # the log-SNR must strictly decrease along the plan
        with pytest.raises(ValueError):
            dpmpp_2m_table(abar, np.array(bad, dtype=np.int32))
    with pytest.raises(ValueError):
        dpmpp_2m_table(abar, np.arange(30), "velocity")
    with pytest.raises(ValueError):
        dpmpp_2m_table(abar, np.arange(30), "v_prediction", sqrt_alphas_cumprod=np.ones(29, dtype=np.float32))
    flat = np.r_[abar[:10], abar[9], abar[10:]].astype(np.float32)      # a schedule with a repeated level
    with pytest.raises(ValueError):
        dpmpp_2m_table(flat, np.array([3, 9, 10, 20], dtype=np.int32))
    one = np.r_[np.float32(1.0), abar].astype(np.float32)               # abar = 1: an infinite log-SNR
    with pytest.raises(ValueError):
        dpmpp_2m_table(one, np.array([0, 5, 9], dtype=np.int32))
    dpmpp_2m_table(abar, np.arange(30))
    dpmpp_2m_table(abar, np.array([29], dtype=np.int32))


# ---- logsnr_timesteps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_,S", [(1000, 1), (1000, 5), (1000, 10), (1000, 50), (1000, 400), (1000, 999), (1000, 1000), (100, 10), (8, 8), (8, 3)])
def test_logsnr_timesteps(T_, S):
    abar = cosine_abar(T_)
    tau = logsnr_timesteps(abar, S)
    assert tau.dtype == np.int32 and tau.shape == (S,)
    assert (np.diff(tau) > 0).all() and tau[-1] == T_ - 1 and tau[0] >= 0
    if S == T_:
        assert np.array_equal(tau, np.arange(T_))
    # a plan like any other
    ddim_step_table(abar, tau, 0.0)
    dpmpp_2m_table(abar, tau)
    assert np.array_equal(logsnr_timesteps(abar.numpy(), S), tau)


def test_logsnr_timesteps_rejects():
    abar = cosine_abar(100)
    for S in (0, -3, 101):
        with pytest.raises(ValueError):
            logsnr_timesteps(abar, S)
    with pytest.raises(ValueError):
        logsnr_timesteps(np.r_[np.float32(1.0), abar.numpy()], 5)


# ---- solver quality on a Gaussian toy ---------------------------------------------------------------------------------------------
# data x_0 ~ N(mu, s^2) per coordinate: the exact denoiser is x0^(x, t) = mu + s^2 alpha (x - alpha mu)/(alpha^2 s^2 + sigma^2), and the
# probability-flow ODE from x_T at abar_T has the closed-form solution x_0 = mu + s (x_T - sqrt(abar_T) mu)/sqrt(abar_T s^2 + 1 - abar_T)
TOY_MU = np.array([-1.0, 0.5, 2.0])[:, None, None]
TOY_S = np.array([0.25, 0.5, 1.0])[None, :, None]
TOY_XT = np.linspace(-3.0, 3.0, 13)[None, None, :]


def toy_error(abar32, taus, solver):
    """Max error of the S-step chain over the toy's (mu, s, x_T) grid against the exact solution, in float64."""
    abar = np.asarray(abar32, dtype=np.float32).astype(np.float64)
    if solver == "ddim":
        tab = ddim_x0_table(abar32, taus, 0.0).astype(np.float64)
        hist = np.zeros(len(taus))
    else:
        _, tab, hist = dpmpp_2m_table(abar32, taus)
        tab, hist = tab.astype(np.float64), hist.astype(np.float64)
    x = np.broadcast_to(TOY_XT, (3, 3, TOY_XT.shape[-1])).copy()
    prev = np.zeros_like(x)
    for s in reversed(range(len(taus))):
        a = abar[taus[s]]
        x0 = TOY_MU + TOY_S ** 2 * math.sqrt(a) * (x - math.sqrt(a) * TOY_MU) / (a * TOY_S ** 2 + 1.0 - a)
        x = tab[s, 2] * x0 + tab[s, 3] * x + hist[s] * prev
        prev = x0
    aT = abar[taus[-1]]
    exact = TOY_MU + TOY_S * (TOY_XT - math.sqrt(aT) * TOY_MU) / np.sqrt(aT * TOY_S ** 2 + 1.0 - aT)
    return np.abs(x - exact).max()


def test_solver_quality_on_the_gaussian_toy():
    abar = cosine_abar().numpy()
    for S in (5, 10, 20, 40):
        uni = ddim_timesteps(1000, S)
        e_ddim, e_2m = toy_error(abar, uni, "ddim"), toy_error(abar, uni, "dpmpp_2m")
        e_log = toy_error(abar, logsnr_timesteps(abar, S), "dpmpp_2m")
        print(f"S={S}: DDIM uniform {e_ddim:.4f}, 2M uniform {e_2m:.4f}, 2M logsnr {e_log:.4f}")
        assert e_2m < e_ddim, S
        if S >= 10:
            assert e_log < e_ddim, S


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains():
    m = cpu_model()
    c = make_case(m)
    lo, hi = mixed_bounds()
    sd64, sd32 = model_sd(m, torch.float64), model_sd(m, torch.float32)

    def run(dtype, variant=None, lo_=lo, hi_=hi, known=None):
        return dpmpp_chain(m, c["cond"], c["x_start"], lambda s: c["zs"][len(PLAN) - 1 - s], PLAN, lo_, hi_, dtype, variant,
                           sd=sd64 if dtype == torch.float64 else sd32, known=known)
    kn = c["known"]["thirty_percent"]
    return lo, hi, dict(ref=run(torch.float64), f32=run(torch.float32), wrong={v: run(torch.float64, v) for v in VARIANTS},
                        free=run(torch.float64, None, None, None), free32=run(torch.float32, None, None, None),
                        free_wrong={v: run(torch.float64, v, None, None) for v in ("no_history", "stale_history")},
                        known=run(torch.float64, known=kn), known32=run(torch.float32, known=kn), kn=kn)


def test_restatement(chains):
    """The result lies inside the bounds exactly; float32 (the library's tables and operation order) agrees with float64 at the chain
    tolerance, bounded, unbounded and around observed values; each wrong chain does not."""
    lo, hi, r = chains
    lo_t, hi_t = torch.from_numpy(lo), torch.from_numpy(hi)
    for name in ("ref", "f32"):
        v = r[name]
        assert bool((v >= lo_t.to(v.dtype)).all()) and bool((v <= hi_t.to(v.dtype)).all()), name
    for ref, f32, name in ((r["ref"], r["f32"], "bounded"), (r["free"], r["free32"], "unbounded"), (r["known"], r["known32"], "known")):
        tol = tol_of(ref)
        err = (f32.double() - ref).abs().max().item()
        print(f"{name}: max|ref|={ref.abs().max().item():.3e} tol={tol:.3e} fp32-fp64={err:.3e}")
        assert err <= tol, name
    obs = ~torch.isnan(r["kn"])
    assert torch.equal(r["known"][obs], r["kn"].double()[obs]) and torch.equal(r["known32"][obs], r["kn"][obs])
    tol = tol_of(r["ref"])
    for v, wrong in r["wrong"].items():
        d = (wrong - r["ref"]).abs().max().item()
        print(f"  {v}: {d:.3e} ({d / tol:.0f} x tol)")
        assert d > tol, v
    tol = tol_of(r["free"])
    for v, wrong in r["free_wrong"].items():
        d = (wrong - r["free"]).abs().max().item()
        print(f"  unbounded {v}: {d:.3e} ({d / tol:.0f} x tol)")
        assert d > tol, v
    assert (r["free"] - r["ref"]).abs().max().item() > tol_of(r["ref"])          # the clamp is active
