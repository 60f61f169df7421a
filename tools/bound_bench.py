"""The likelihood sweep's rate and the price of its row-loss launch, one JSON line per measurement.

  --mode sweep    rows/s ((timestep, patient) pairs per second) of model.variational_bound at D = 2000 for n = 4096 x S = 32 and
                  n = 100 000 x S = 8, for every --bound-rows value (the measurement behind the library's default): each shape is
                  warmed up once per cap, then the caps ALTERNATE over --rounds rounds; a line reports the median and the spread.
  --mode launch   the per-row call (model.row_sq_error: q_sample of pairs, forward trunk, output_proj + EpiRowSq, the slot sum)
                  against the loss-only training call (output_proj + EpiMse, no dout) at the same --rows, alternating windows of
                  whole calls.  The two launches themselves are kernel times: run this mode under
                  `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bound_bench.py --mode launch --rounds 1 --window 0.3`
                  and compare the gemm kernels whose names carry EpiRowSq (+ k_rowsq_reduce) and EpiMse in the statistics.

    python tools/bound_bench.py [--mode sweep,launch] [--bound-rows 8192,16384,32768,65536] [--rows 32768] [--rounds 5] [--window 1.0]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel  # noqa: E402
from osteosarcoma_diffusionmodel_amd.train import _loss_fwd_bwd  # noqa: E402

DIMS = (50, 1900, 50, 3)
SHAPES = ((4096, 32), (100000, 8))


def model():
    conf = {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": 1000, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"}}
    torch.manual_seed(0)
    return BiologyAwareDiffusionModel(*DIMS, conf).cuda().eval()


def cohort(n):
    g = torch.Generator(device="cuda").manual_seed(42)
    x = torch.randn(n, sum(DIMS[:3]), device="cuda", generator=g)
    x[:, :DIMS[0]] = (torch.rand(n, DIMS[0], device="cuda", generator=g) < 0.5).float()
    return x, torch.randn(n, DIMS[3], device="cuda", generator=g)


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


def sweep(m, caps, rounds, window):
    for n, S in SHAPES:
        x, c = cohort(n)
        def call():
            return m.variational_bound(x, c, num_timesteps=S, seed=7)
        wins = {cap: [] for cap in caps}
        for cap in caps:
            m.bound_rows = cap
            call()
        for _ in range(rounds):
            for cap in caps:
                m.bound_rows = cap
                wins[cap].append(timed(call, window))
        for cap in caps:
            w = sorted(wins[cap])
            report({"mode": "sweep", "n": n, "S": S, "bound_rows": cap}, wins[cap], rows_per_s=round(n * S / w[len(w) // 2]))
        del x, c
        torch.cuda.empty_cache()


def launch(m, rows, rounds, window):
    x, c = cohort(rows)
    t = torch.randint(0, 1000, (rows,), device="cuda")
    calls = {"row_sq_error": lambda: m.row_sq_error(x, c, t, seed=7),
             "loss_only": lambda: _loss_fwd_bwd(m, x, c, None, t=t, seed=7)}
    wins = {k: [] for k in calls}
    m.bound_rows = max(rows, 1)
    for fn in calls.values():
        for _ in range(5):
            fn()
    for _ in range(rounds):
        for k, fn in calls.items():
            wins[k].append(timed(fn, window))
    med = {k: report({"mode": "launch", "rows": rows, "call": k}, wins[k]) for k in calls}
    print(json.dumps({"mode": "launch", "rows": rows, "row_sq_error_over_loss_only": round(med["row_sq_error"] / med["loss_only"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="sweep,launch")
    ap.add_argument("--bound-rows", default="8192,16384,32768,65536")
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    m = model()
    if "launch" in args.mode.split(","):
        launch(m, args.rows, args.rounds, args.window)
    if "sweep" in args.mode.split(","):
        sweep(m, [int(v) for v in args.bound_rows.split(",")], args.rounds, args.window)


if __name__ == "__main__":
    main()
