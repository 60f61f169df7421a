"""What the noise map of a counterfactual costs, one JSON line per measurement.

  --mode map      model.invert(method="ddpm") -- one osd_noise_map call: k_q_sample_map, the forward trunk, output_proj + EpiNoiseMap --
                  at D = 2000 for every --shapes entry n x S (S levels, n x (S - 1) rows), against
                    sweep        osd_bound_sweep over the same n x (S - 1) rows: the nearest call the library had before
                    composed     what the map replaces: q_sample per level, predict on the n x S rows, the solve in torch
                    copy         a device copy of rows x D floats: the write the map adds to a loss-only sweep
                  in alternating windows of whole calls; the composed result is also compared with the map's (C z, relative to max|C z|).
  --mode e2e      SyntheticPatientGenerator.counterfactual end to end (upload, transform-free inversion, decode, download) for --patients
                  rows at sampling_steps = 50, strength = 0.6, at D = 2000 and at the reference's dims (62 / 5054 / 26).

    python tools/edit_bench.py [--mode map,e2e] [--shapes 128x31,4096x31] [--patients 100] [--rounds 5] [--window 1.0]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator, _lib as L  # noqa: E402
from osteosarcoma_diffusionmodel_amd.ddim import ddim_step_table  # noqa: E402

DIMS = (50, 1900, 50, 3)
REAL_DIMS = (62, 5054, 26, 3)
T = 1000


def config():
    return {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": T, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"}}


def model(dims=DIMS):
    torch.manual_seed(0)
    return BiologyAwareDiffusionModel(*dims, config()).cuda().eval()


def cohort(n, dims=DIMS):
    g = torch.Generator(device="cuda").manual_seed(42)
    x = torch.randn(n, sum(dims[:3]), device="cuda", generator=g)
    x[:, :dims[0]] = (torch.rand(n, dims[0], device="cuda", generator=g) < 0.5).float()
    return x, torch.randn(n, dims[3], device="cuda", generator=g)


def timed(fn, seconds):
    """Seconds per call over whole calls lasting at least `seconds`, bracketed by device synchronisation."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / n


def report(tag, wins, **extra):
    w = sorted(wins)
    med = w[len(w) // 2]
    print(json.dumps({**tag, "ms_per_call": round(1e3 * med, 4), "ms_min": round(1e3 * w[0], 4), "ms_max": round(1e3 * w[-1], 4),
                      "spread_pct": round(100 * (w[-1] - w[0]) / med, 2), "windows": len(w), **extra}), flush=True)
    return med


def levels_of(S):
    """S strictly increasing levels, 0 first, spread over the lower 60 % of the schedule: the plan of a strength-0.6 edit."""
    return np.unique(np.r_[0, np.linspace(T // 50 - 1, int(0.6 * T) - 1, S - 1).round()]).astype(np.int32)


@torch.no_grad()
def composed(m, x, c, levels, coef, eps):
    """The map from the calls the library had: q_sample per level, one predict over the n x S rows, the solve in torch."""
    n, S = x.shape[0], levels.size
    ys = [m.q_sample(x, torch.full((n,), int(t), device="cuda"), eps[s])[0] for s, t in enumerate(levels)]
    t_rows = torch.as_tensor(np.repeat(levels, n), device="cuda")
    out = m._raw_output(torch.cat(ys), t_rows, c.repeat(S, 1)).view(S, n, -1)
    cz = [ys[s - 1] - (float(coef[s, 0]) * ys[s] + float(coef[s, 1]) * out[s]) for s in range(S - 1, 0, -1)]
    return ys[-1], torch.stack(cz)


@torch.no_grad()
def map_mode(m, shapes, rounds, window):
    for n, S in shapes:
        levels = levels_of(S)
        S = int(levels.size)
        rows, D = n * (S - 1), m.data_dim
        x, c = cohort(n)
        taus, coef = ddim_step_table(m.alphas_cumprod, levels, 1.0, m.prediction_type, sqrt_alphas_cumprod=m.sqrt_alphas_cumprod,
                                     sqrt_one_minus_alphas_cumprod=m.sqrt_one_minus_alphas_cumprod)
        eps = torch.randn(S, n, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        src, dst = torch.empty(rows, D, device="cuda").normal_(), torch.empty(rows, D, device="cuda")

        def invert(noise=None):
            # the plan of invert() is edit_timesteps'; the bench fixes its own levels, so it goes through the entry point itself
            eng = m._engine()
            xs, z = torch.empty_like(x), torch.empty(S - 1, n, D, device="cuda")
            L.check(L.lib().osd_noise_map(eng.handle, L.ptr(x), L.ptr(c), n, taus.ctypes.data, coef.ctypes.data, S, L.ptr(noise), 7, 0,
                                          L.ptr(xs), L.ptr(z)))
            return xs, z

        calls = {"noise_map": invert,
                 "sweep": lambda: m._bound_sweep(x, c, levels[1:], None, 7, 0),
                 "composed": lambda: composed(m, x, c, levels, coef, eps),
                 "copy": lambda: dst.copy_(src)}
        # values first: the composition against the map on the same injected draws
        xs, z = invert(eps)
        xs_c, cz_c = composed(m, x, c, levels, coef, eps)
        cs = torch.tensor([float(coef[S - 1 - k, 2]) for k in range(S - 1)], device="cuda")
        cz = z * cs[:, None, None]
        print(json.dumps({"mode": "map", "n": n, "S": S, "check": "composed vs noise_map",
                          "cz_max_abs_diff_over_max": float((cz - cz_c).abs().max() / cz_c.abs().max()),
                          "x_start_max_abs_diff": float((xs - xs_c).abs().max())}), flush=True)
        del xs, z, xs_c, cz_c, cz
        wins = {k: [] for k in calls}
        for fn in calls.values():
            for _ in range(3):
                fn()
        for _ in range(rounds):
            for k, fn in calls.items():
                wins[k].append(timed(fn, window))
        tag = {"mode": "map", "n": n, "S": S, "rows": rows, "D": D}
        med = {k: report({**tag, "call": k}, wins[k]) for k in calls}
        print(json.dumps({**tag, "noise_map_over_sweep": round(med["noise_map"] / med["sweep"], 4),
                          "noise_map_minus_sweep_over_copy": round((med["noise_map"] - med["sweep"]) / med["copy"], 4),
                          "composed_over_noise_map": round(med["composed"] / med["noise_map"], 4),
                          "copy_GBps": round(2 * rows * D * 4 / med["copy"] / 1e9, 1)}), flush=True)
        del x, c, eps, src, dst
        torch.cuda.empty_cache()


def e2e_mode(patients, rounds, window):
    for dims in (DIMS, REAL_DIMS):
        m = model(dims)
        gen = SyntheticPatientGenerator(m, config(), device="cuda")
        x, c = cohort(patients, dims)
        feats, cond = x.cpu().numpy(), c.cpu().numpy()

        def call():
            return gen.counterfactual(feats, cond, {"metastasis_at_diagnosis": 1}, keep={"mutations": True}, sampling_steps=50, strength=0.6, seed=3)
        for _ in range(3):
            call()
        wins = [timed(call, window) for _ in range(rounds)]
        report({"mode": "e2e", "patients": patients, "D": int(sum(dims[:3])), "sampling_steps": 50, "strength": 0.6, "last_sampler": m.last_sampler},
               wins)
        del m, gen
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="map,e2e")
    ap.add_argument("--shapes", default="128x31,4096x31")
    ap.add_argument("--patients", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    modes = args.mode.split(",")
    if "map" in modes:
        map_mode(model(), [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")], args.rounds, args.window)
    if "e2e" in modes:
        e2e_mode(args.patients, args.rounds, args.window)


if __name__ == "__main__":
    main()
