"""Throughput of the strided DDIM sampler against the DDPM chain, in patients/s (one JSON line per case).

Each case runs once to warm up (engine creation, weight packing, graph capture), then three timed repeats, each bracketed
by torch.cuda.synchronize(); the line reports the median and the spread (min, max) of the three.

  reference   3 x 1000 patients at dims 62 / 5054 / 26 through SyntheticPatientGenerator.generate_scenarios,
              S = 50, S = 100 and the T = 1000 DDPM chain
  headline    100 000 patients at D = 2000 (50 / 1900 / 50), S = 50
  eta         eta = 0 against eta = 1 at S = 50, 100 000 patients at D = 2000, on the per-layer kernels and on the workspace
              chain kernel (decides whether the posterior epilogues' skip of the Philox draw at C = 0 pays)

    python tools/ddim_bench.py [--cases reference,headline,eta] [--repeats 3]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator  # noqa: E402


def config(T=1000):
    return {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": T, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"}}


def timed(fn, patients, repeats):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(patients / (time.perf_counter() - t0))
    runs.sort()
    return {"patients_per_s": round(runs[len(runs) // 2], 1), "min": round(runs[0], 1), "max": round(runs[-1], 1),
            "spread_pct": round(100 * (runs[-1] - runs[0]) / runs[len(runs) // 2], 2)}


def emit(case, **kw):
    print(json.dumps({"case": case, **kw}), flush=True)


def reference(repeats):
    torch.manual_seed(0)
    m = BiologyAwareDiffusionModel(62, 5054, 26, 3, config()).cuda().eval()
    gen = SyntheticPatientGenerator(m, config(), device="cuda")
    scen = [{"name": n, "conditions": c} for n, c in (
        ("good_prognosis", {"survival_time": 2000, "event_occurred": 0, "metastasis_at_diagnosis": 0}),
        ("poor_prognosis", {"survival_time": 300, "event_occurred": 1, "metastasis_at_diagnosis": 1}),
        ("intermediate", {"survival_time": 800, "event_occurred": 0, "metastasis_at_diagnosis": 1}))]
    for steps in (50, 100, None):
        r = timed(lambda: gen.generate_scenarios(scen, 1000, seed=1, sampling_steps=steps), 3000, repeats)
        emit("reference_3x1000", sampling_steps=steps or "ddpm", engine=m.last_sampler, variant=m.last_chain_variant, **r)


def headline_model():
    torch.manual_seed(0)
    return BiologyAwareDiffusionModel(50, 1900, 50, 3, config()).cuda().eval()


def headline(repeats, m):
    n = 100_000
    cond = torch.randn(n, 3, device="cuda")
    r = timed(lambda: m.sample(cond, n, seed=1, num_inference_steps=50), n, repeats)
    emit("headline_100k_D2000", sampling_steps=50, engine=m.last_sampler, variant=m.last_chain_variant, **r)


def eta(repeats, m):
    n = 100_000
    cond = torch.randn(n, 3, device="cuda")
    for sampler, variant in (("graph", None), ("chain", "workspace")):
        m.sampler, m.chain_variant = sampler, variant
        for e in (0.0, 1.0):
            r = timed(lambda: m.sample(cond, n, seed=1, num_inference_steps=50, eta=e), n, repeats)
            emit("eta_100k_D2000", sampling_steps=50, eta=e, engine=m.last_sampler, variant=m.last_chain_variant, **r)
    m.sampler, m.chain_variant = "auto", None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="reference,headline,eta")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    cases = args.cases.split(",")
    with torch.no_grad():
        if "reference" in cases:
            reference(args.repeats)
        if "headline" in cases or "eta" in cases:
            m = headline_model()
            if "headline" in cases:
                headline(args.repeats, m)
            if "eta" in cases:
                eta(args.repeats, m)


if __name__ == "__main__":
    main()
