"""Price of known-feature conditioning: a chain around observed values against the unconstrained chain, in ms per step (one JSON
line per run), both on the per-layer engine (sampler = "graph", hipGraph replay).  The unconstrained per-layer kernels are
untouched by the feature, so that column is also the figure of the commit before it.

Each run warms up once (engine creation, weight packing, graph capture), then `--repeats` timed repeats, each bracketed by
torch.cuda.synchronize(); a line reports the median and the spread (min, max).  S = 50, eta = 0 throughout: the known chain then
draws z at every step for its observed elements, the unconstrained chain draws nothing -- the comparison includes that.

  mutations   100 000 patients at D = 2000 (50 / 1900 / 50), the mutation block observed
  thirty      the same, 30 % of all elements observed
  reference   3 x 1000 patients at dims 62 / 5054 / 26 through SyntheticPatientGenerator.generate_scenarios (input_splitk = -1, the
              generator's setting, on both sides), the mutation block observed

The last line of a case holds the ratio; the reference case adds the same chains through model.sample with the observation array
already on the device (the step alone, without the generator's per-call host preparation).

    python tools/known_bench.py [--cases mutations,thirty,reference] [--repeats 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator  # noqa: E402

STEPS = 50


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


def large(case, pattern, repeats):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(50, 1900, 50, 3, config()).cuda().eval()
    m.sampler = "graph"
    n = 100_000
    cond = torch.randn(n, 3, device="cuda")
    known = torch.full((n, m.data_dim), float("nan"), device="cuda")
    if pattern == "mutations":
        known[:, :50] = (torch.rand(n, 50, device="cuda") < 0.3).float()
    else:
        pick = torch.rand(n, m.data_dim, device="cuda") < 0.3
        known[pick] = torch.randn(n, m.data_dim, device="cuda")[pick]
    res = {}
    for run, kn in (("known", known), ("unconstrained", None)):
        res[run] = timed(lambda: m.sample(cond, n, seed=1, num_inference_steps=STEPS, known=kn), repeats)
        emit(case, run=run, rows=n, observed_fraction=0.0 if kn is None else round(float((~torch.isnan(kn)).float().mean()), 4),
             engine=m.last_sampler, **res[run])
    emit(case, run="ratio", known_over_unconstrained=round(res["known"]["ms_per_step"] / res["unconstrained"]["ms_per_step"], 4))


def reference(repeats):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(62, 5054, 26, 3, config()).cuda().eval()
    gen = SyntheticPatientGenerator(m, config(), device="cuda")          # sets input_splitk = -1
    m.sampler = "graph"
    scen = [{"name": n, "conditions": c} for n, c in (
        ("good_prognosis", {"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0}),
        ("poor_prognosis", {"survival_time": 300, "event_occurred": 1, "metastasis_at_diagnosis": 1}),
        ("intermediate", {"survival_time": 800, "event_occurred": 0, "metastasis_at_diagnosis": 1}))]
    case = "reference_3x1000_mutations"
    mut = (np.random.default_rng(0).random((1000, 62)) < 0.3).astype(np.float32)
    res = {}
    for run, kn in (("known", {"mutations": mut}), ("unconstrained", None)):
        res[run] = timed(lambda: gen.generate_scenarios(scen, 1000, seed=1, sampling_steps=STEPS, known=kn), repeats)
        emit(case, run=run, rows=3000, engine=m.last_sampler, **res[run])
    emit(case, run="ratio", known_over_unconstrained=round(res["known"]["ms_per_step"] / res["unconstrained"]["ms_per_step"], 4))
    # the same chains through model.sample with the observations already on the device: the step alone, without the generator's
    # per-call preparation of the observation array (assemble_known on the host, one upload, the repeat per scenario)
    cond = torch.cat([gen.create_conditions(1000, sc["conditions"]) for sc in scen], dim=0)
    known = torch.full((3000, m.data_dim), float("nan"), device="cuda")
    known[:, :62] = torch.from_numpy(mut).cuda().repeat(3, 1)
    for run, kn in (("known_on_device", known), ("unconstrained_model_sample", None)):
        res[run] = timed(lambda: m.sample(cond, 3000, seed=1, num_inference_steps=STEPS, known=kn), repeats)
        emit(case, run=run, rows=3000, engine=m.last_sampler, **res[run])
    emit(case, run="ratio_on_device",
         known_over_unconstrained=round(res["known_on_device"]["ms_per_step"] / res["unconstrained_model_sample"]["ms_per_step"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="mutations,thirty,reference")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cases = args.cases.split(",")
    with torch.no_grad():
        if "mutations" in cases:
            large("100k_D2000_mutations", "mutations", args.repeats)
        if "thirty" in cases:
            large("100k_D2000_thirty_percent", "thirty", args.repeats)
        if "reference" in cases:
            reference(args.repeats)


if __name__ == "__main__":
    main()
