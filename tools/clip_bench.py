"""Price of clipping the predicted x0 inside the sampling step: the clipped chain against the unclipped chain, in ms per step (one JSON
line per run), both on the per-layer engine (sampler = "graph", hipGraph replay).  The unclipped per-layer kernels are untouched by
the feature, so that column is also the figure of the commit before it.

Each run warms up once (engine creation, weight packing, graph capture), then `--repeats` timed repeats, each bracketed by
torch.cuda.synchronize(); a line reports the median and the spread (min, max).  S = 50, eta = 0 throughout, unguided and at
guidance_scale = 7.5 (the setting the clamp is the usual companion of).  Bounds: mutations [0, 1], expression [-4, 4], pathways free.

  large       100 000 patients at D = 2000 (50 / 1900 / 50) through model.sample
  reference   3 x 1000 patients at dims 62 / 5054 / 26 through model.sample on the concatenated conditions (input_splitk = -1, the
              generator's setting, on both sides)

The last line of a case holds the ratio.

    python tools/clip_bench.py [--cases large,reference] [--repeats 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator  # noqa: E402

STEPS = 50
BOUNDS = {"mutations": (0.0, 1.0), "expression": (-4.0, 4.0)}
NULL_CONDITION = [0.0, 0.0, 0.0]


def config(T=1000):
    return {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": T, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"}}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    runs.sort()
    med = runs[len(runs) // 2]
    return {"ms_per_step": round(1e3 * med / STEPS, 4), "ms_per_step_min": round(1e3 * runs[0] / STEPS, 4),
            "ms_per_step_max": round(1e3 * runs[-1] / STEPS, 4), "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2)}


def emit(case, **kw):
    print(json.dumps({"case": case, **kw}), flush=True)


def compare(case, m, cond, repeats):
    n = cond.shape[0]
    for w in (1.0, 7.5):
        res = {}
        for run, bounds in (("clipped", BOUNDS), ("unclipped", False)):
            res[run] = timed(lambda: m.sample(cond, n, seed=1, num_inference_steps=STEPS, guidance_scale=w, x0_bounds=bounds), repeats)
            emit(case, run=run, guidance_scale=w, rows=n, engine=m.last_sampler, **res[run])
        emit(case, run="ratio", guidance_scale=w, clipped_over_unclipped=round(res["clipped"]["ms_per_step"] / res["unclipped"]["ms_per_step"], 4))


def large(repeats):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(50, 1900, 50, 3, config()).cuda().eval()
    m.sampler = "graph"
    m.null_condition = NULL_CONDITION
    compare("100k_D2000", m, torch.randn(100_000, 3, device="cuda"), repeats)


def reference(repeats):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(62, 5054, 26, 3, config()).cuda().eval()
    gen = SyntheticPatientGenerator(m, config(), device="cuda")          # sets input_splitk = -1
    m.sampler = "graph"
    m.null_condition = NULL_CONDITION
    scen = ({"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0},
            {"survival_time": 300, "event_occurred": 1, "metastasis_at_diagnosis": 1},
            {"survival_time": 800, "event_occurred": 0, "metastasis_at_diagnosis": 1})
    cond = torch.cat([gen.create_conditions(1000, sc) for sc in scen], dim=0)
    compare("reference_3x1000", m, cond, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="large,reference")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cases = args.cases.split(",")
    with torch.no_grad():
        if "large" in cases:
            large(args.repeats)
        if "reference" in cases:
            reference(args.repeats)


if __name__ == "__main__":
    main()
