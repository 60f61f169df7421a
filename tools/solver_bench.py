"""Price and pay-off of the DPM-Solver++(2M) multistep sampler: the 2M chain against the clipped DDIM chain with the same bounds, in ms
per step (one JSON line per run), both on the per-layer engine (sampler = "graph", hipGraph replay).  The clipped chain's kernels are
untouched by the feature, so that column is also the figure of the commit before it.

Each run warms up once (engine creation, weight packing, graph capture), then `--repeats` timed repeats, each bracketed by
torch.cuda.synchronize(); a line reports the median and the spread (min, max).  S = 50, eta = 0, unguided and at guidance_scale = 7.5.
Bounds: mutations [0, 1], expression [-4, 4], pathways free.

  large       100 000 patients at D = 2000 (50 / 1900 / 50) through model.sample
  reference   3 x 1000 patients at dims 62 / 5054 / 26 through model.sample on the concatenated conditions (input_splitk = -1, the
              generator's setting, on both sides)
  endtoend    the reference workload, unbounded and unguided, in patients/s: 2M at S = 20 against DDIM at S = 50 and at S = 20

The last line of a case holds the ratio.

    python tools/solver_bench.py [--cases large,reference,endtoend] [--repeats 3]
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
    """Seconds of `repeats` runs after one warm-up, sorted."""
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    return sorted(runs)


def per_step(runs, steps):
    med = runs[len(runs) // 2]
    return {"ms_per_step": round(1e3 * med / steps, 4), "ms_per_step_min": round(1e3 * runs[0] / steps, 4),
            "ms_per_step_max": round(1e3 * runs[-1] / steps, 4), "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2)}


def emit(case, **kw):
    print(json.dumps({"case": case, **kw}), flush=True)


def compare(case, m, cond, repeats):
    n = cond.shape[0]
    for w in (1.0, 7.5):
        res = {}
        for run, solver in (("dpmpp_2m", "dpmpp_2m"), ("clipped_ddim", "ddim")):
            res[run] = per_step(timed(lambda: m.sample(cond, n, seed=1, num_inference_steps=STEPS, guidance_scale=w, x0_bounds=BOUNDS,
                                                       solver=solver), repeats), STEPS)
            emit(case, run=run, guidance_scale=w, rows=n, engine=m.last_sampler, **res[run])
        emit(case, run="ratio", guidance_scale=w, dpmpp_2m_over_clipped_ddim=round(res["dpmpp_2m"]["ms_per_step"] / res["clipped_ddim"]["ms_per_step"], 4))


def large(repeats):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(50, 1900, 50, 3, config()).cuda().eval()
    m.sampler = "graph"
    m.null_condition = NULL_CONDITION
    compare("100k_D2000", m, torch.randn(100_000, 3, device="cuda"), repeats)


def reference_model():
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(62, 5054, 26, 3, config()).cuda().eval()
    gen = SyntheticPatientGenerator(m, config(), device="cuda")          # sets input_splitk = -1
    m.null_condition = NULL_CONDITION
    scen = ({"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0},
            {"survival_time": 300, "event_occurred": 1, "metastasis_at_diagnosis": 1},
            {"survival_time": 800, "event_occurred": 0, "metastasis_at_diagnosis": 1})
    return m, torch.cat([gen.create_conditions(1000, sc) for sc in scen], dim=0)


def reference(repeats):
    m, cond = reference_model()
    m.sampler = "graph"
    compare("reference_3x1000", m, cond, repeats)


def endtoend(repeats):
    """Patients/s of whole model.sample calls on the default engine: what a user who trades steps for a better solver gets."""
    m, cond = reference_model()
    n = cond.shape[0]
    for run, kw in (("dpmpp_2m_S20", dict(num_inference_steps=20, solver="dpmpp_2m")), ("ddim_S50", dict(num_inference_steps=50)),
                    ("ddim_S20", dict(num_inference_steps=20))):
        runs = timed(lambda: m.sample(cond, n, seed=1, **kw), repeats)
        med = runs[len(runs) // 2]
        emit("endtoend_3x1000", run=run, rows=n, engine=m.last_sampler, patients_per_s=round(n / med, 1), patients_per_s_min=round(n / runs[-1], 1),
             patients_per_s_max=round(n / runs[0], 1), spread_pct=round(100 * (runs[-1] - runs[0]) / med, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="large,reference,endtoend")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cases = args.cases.split(",")
    with torch.no_grad():
        if "large" in cases:
            large(args.repeats)
        if "reference" in cases:
            reference(args.repeats)
        if "endtoend" in cases:
            endtoend(args.repeats)


if __name__ == "__main__":
    main()
