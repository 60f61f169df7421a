"""Price of classifier-free guidance: guided against unguided sampling in rows/s (rows the chain was asked for: patients of a guided
run) and ms per step (one JSON line per run).

Each run warms up once (engine creation, weight packing, graph capture), then `--repeats` timed repeats, each bracketed by
torch.cuda.synchronize(); a line reports the median and the spread (min, max).  S = 50, eta = 0 throughout.

  headline    100 000 patients at D = 2000 (50 / 1900 / 50) through model.sample
  reference   3 x 1000 patients at dims 62 / 5054 / 26 through SyntheticPatientGenerator.generate_scenarios (input_splitk = -1, the
              generator's setting, on every side)

Per case, on the per-layer engine (sampler = "graph", hipGraph replay): the guided chain on n patients, the unguided chain on n
rows, and the unguided chain on 2 n rows -- what two full passes per step cost, the figure the guided step has to beat (the GEMM
count predicts 0.80 of it at D = 2000, 0.69 at D = 5142).  Then the unguided chain on n rows on whatever engine "auto" picks: the
real price of guidance_scale != 1 to a user.  The last line of a case holds the ratios.

    python tools/guidance_bench.py [--cases headline,reference] [--repeats 3] [--scale 3.0]
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


def config(T=1000):
    return {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": T, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion",
                      "null_condition": [0.0, 0.0, 0.0]}}


def timed(fn, rows, repeats):
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
    return {"rows_per_s": round(rows / med, 1), "ms_per_step": round(1e3 * med / STEPS, 4),
            "ms_per_step_min": round(1e3 * runs[0] / STEPS, 4), "ms_per_step_max": round(1e3 * runs[-1] / STEPS, 4),
            "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2)}


def emit(case, **kw):
    print(json.dumps({"case": case, **kw}), flush=True)


def ratios(case, guided, plain_n, plain_2n, auto_n):
    emit(case, run="ratios", guided_over_unguided_2n=round(guided["ms_per_step"] / plain_2n["ms_per_step"], 4),
         guided_over_unguided_n=round(guided["ms_per_step"] / plain_n["ms_per_step"], 4),
         guided_over_auto_n=round(guided["ms_per_step"] / auto_n["ms_per_step"], 4))


def headline(repeats, scale):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(50, 1900, 50, 3, config()).cuda().eval()
    n = 100_000
    cond = torch.randn(2 * n, 3, device="cuda")
    cond_n = cond[:n].contiguous()
    case = "headline_100k_D2000"
    m.sampler = "graph"
    res = {}
    for run, c, rows, w in (("guided", cond_n, n, scale), ("unguided_n", cond_n, n, 1.0), ("unguided_2n", cond, 2 * n, 1.0)):
        res[run] = timed(lambda: m.sample(c, rows, seed=1, num_inference_steps=STEPS, guidance_scale=w), rows, repeats)
        emit(case, run=run, rows=rows, guidance_scale=w, engine=m.last_sampler, variant=m.last_chain_variant, **res[run])
    m.sampler = "auto"
    res["auto_n"] = timed(lambda: m.sample(cond_n, n, seed=1, num_inference_steps=STEPS), n, repeats)
    emit(case, run="unguided_n_auto", rows=n, guidance_scale=1.0, engine=m.last_sampler, variant=m.last_chain_variant, **res["auto_n"])
    ratios(case, res["guided"], res["unguided_n"], res["unguided_2n"], res["auto_n"])


def reference(repeats, scale):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(62, 5054, 26, 3, config()).cuda().eval()
    gen = SyntheticPatientGenerator(m, config(), device="cuda")          # sets input_splitk = -1
    scen = [{"name": n, "conditions": c} for n, c in (
        ("good_prognosis", {"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0}),
        ("poor_prognosis", {"survival_time": 300, "event_occurred": 1, "metastasis_at_diagnosis": 1}),
        ("intermediate", {"survival_time": 800, "event_occurred": 0, "metastasis_at_diagnosis": 1}))]
    case = "reference_3x1000"
    m.sampler = "graph"
    res = {}
    for run, per, w in (("guided", 1000, scale), ("unguided_n", 1000, 1.0), ("unguided_2n", 2000, 1.0)):
        res[run] = timed(lambda: gen.generate_scenarios(scen, per, seed=1, sampling_steps=STEPS, guidance_scale=w), 3 * per, repeats)
        emit(case, run=run, rows=3 * per, guidance_scale=w, engine=m.last_sampler, variant=m.last_chain_variant, **res[run])
    m.sampler = "auto"
    res["auto_n"] = timed(lambda: gen.generate_scenarios(scen, 1000, seed=1, sampling_steps=STEPS), 3000, repeats)
    emit(case, run="unguided_n_auto", rows=3000, guidance_scale=1.0, engine=m.last_sampler, variant=m.last_chain_variant, **res["auto_n"])
    ratios(case, res["guided"], res["unguided_n"], res["unguided_2n"], res["auto_n"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,reference")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=3.0)
    args = ap.parse_args()
    cases = args.cases.split(",")
    with torch.no_grad():
        if "headline" in cases:
            headline(args.repeats, args.scale)
        if "reference" in cases:
            reference(args.repeats, args.scale)


if __name__ == "__main__":
    main()
