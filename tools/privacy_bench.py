"""Rate of the privacy audit's nearest-record pass against the MMD's RBF rectangle, on one GPU from one build (one JSON line per
measurement).

  nearest   osd_val_nearest, n queries x n references at D = 2000: row norms, the Gram GEMM with the min epilogue (EpiNearest),
            the refine pass
  rbf_sum   osd_val_rbf_sum on the same rectangle with distinct operands (no triangular schedule): row norms and the Gram GEMM
            with the exp + sum epilogue -- the yardstick
  audit     BiologicalValidator.privacy_audit end to end on three n-row cohorts: four nearest passes plus the host summary

Each size warms both calls up once, then times `--repeats` repeats of each, alternating the two so that a drift of the machine hits
both alike; every repeat is bracketed by torch.cuda.synchronize().  A line reports the median, min and max and the spread
(max - min) / median; TFLOP/s counts the 2 n^2 D operations of the Gram product over the whole call (allocation, row norms and, for
nearest, the refine pass included).  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/privacy_bench.py [--sizes 16384,125000] [--repeats 5] [--audit-sizes 16384,125000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402

D = 2000


def stats(runs, flop=None):
    runs = sorted(runs)
    med = runs[len(runs) // 2]
    out = {"ms": round(1e3 * med, 3), "ms_min": round(1e3 * runs[0], 3), "ms_max": round(1e3 * runs[-1], 3),
           "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2), "repeats": len(runs)}
    if flop is not None:
        out["tflops"] = round(flop / med / 1e12, 2)
        out["tflops_best"] = round(flop / runs[0] / 1e12, 2)
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cohort(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, D, device="cuda", generator=g)
    x[:, :50] = (torch.rand(n, 50, device="cuda", generator=g) < 0.3).float()        # the mutation block
    return x


def rectangle(n, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    q, r = cohort(n, 1), cohort(n, 2)
    calls = {"nearest": lambda: k.nearest(q, r), "rbf_sum": lambda: k.rbf_sum(q, r, 1.0 / D)}
    for fn in calls.values():
        fn()
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    flop = 2.0 * n * n * D
    res = {name: stats(v, flop) for name, v in runs.items()}
    for name, v in res.items():
        print(json.dumps({"case": name, "queries": n, "references": n, "D": D, **v}), flush=True)
    print(json.dumps({"case": "ratio", "rows": n, "nearest_over_rbf_sum_time": round(res["nearest"]["ms"] / res["rbf_sum"]["ms"], 4),
                      "larger_spread_pct": max(res["nearest"]["spread_pct"], res["rbf_sum"]["spread_pct"])}), flush=True)


def audit(n, repeats):
    val = BiologicalValidator({"evaluation": {}})
    train, hold, synth = cohort(n, 3), cohort(n, 4), cohort(n, 5)
    synth[: n // 100] = train[: n // 100]                    # one exact copy in a hundred
    box = {}

    def run():
        box["res"] = val.privacy_audit(train, synth, hold)

    run()
    runs = [clock(run) for _ in range(repeats)]
    print(json.dumps({"case": "audit", "rows_per_cohort": n, "D": D, **stats(runs),
                      "exact_copy_fraction": box["res"]["privacy_exact_copy_fraction"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,125000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--audit-sizes", default="16384,125000", help="rows per cohort of the end-to-end audit; empty skips it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("privacy_bench measures on a GPU: none found")
    for n in [int(s) for s in args.sizes.split(",") if s]:
        rectangle(n, args.repeats)
    for n in [int(s) for s in args.audit_sizes.split(",") if s]:
        audit(n, args.repeats)


if __name__ == "__main__":
    main()
