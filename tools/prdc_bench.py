"""Cost of the k-nearest-neighbour and ball-count passes behind precision / recall / density / coverage against the two existing
passes over the same rectangle, on one GPU from one build (one JSON line per measurement).

  knn_k1 / knn_k5 / knn_k16   osd_val_knn, n queries x n references at D = 2000: row norms, the Gram GEMM with the k-best epilogue
                              (EpiKnn; a seeding launch over the leading 512 reference rows, then the rest), refine and sort
  ball_counts                 osd_val_ball_counts with both radii (EpiBallCount); the radii are the queries' and the references'
                              5th-neighbour radii, so the counts are of the size the metrics see
  nearest, rbf_sum            osd_val_nearest and osd_val_rbf_sum on the same operands -- the yardsticks (tools/privacy_bench.py)
  prdc                        BiologicalValidator.fidelity_diversity end to end on two n-row cohorts: two knn passes, two count passes

Each size warms every call up once, then times `--repeats` rounds; a round runs every call once, so the calls alternate and a drift
of the machine hits all alike; every call is bracketed by torch.cuda.synchronize().  A line reports the median, min and max and the
spread (max - min) / median; TFLOP/s counts the 2 n^2 D operations of the Gram product over the whole call (allocation, row norms,
refine and sort included).  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/prdc_bench.py [--sizes 16384,125000] [--repeats 5] [--prdc-sizes 16384,125000]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402
from privacy_bench import D, clock, cohort, stats  # noqa: E402


def rectangle(n, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    q, r = cohort(n, 1), cohort(n, 2)
    own = torch.arange(n, dtype=torch.int32, device="cuda")
    r2_q = k.knn(q, q, 5, own)[0][:, 4].contiguous()
    r2_r = k.knn(r, r, 5, own)[0][:, 4].contiguous()
    box = {}

    def balls():
        box["counts"] = k.ball_counts(q, r, r2_ref=r2_r, r2_query=r2_q)

    calls = {"nearest": lambda: k.nearest(q, r), "knn_k1": lambda: k.knn(q, r, 1), "knn_k5": lambda: k.knn(q, r, 5),
             "knn_k16": lambda: k.knn(q, r, 16), "ball_counts": balls, "rbf_sum": lambda: k.rbf_sum(q, r, 1.0 / D)}
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
    in_ref, in_query = box["counts"]
    print(json.dumps({"case": "counts", "rows": n, "mean_in_ref": round(float(in_ref.double().mean()), 3),
                      "mean_in_query": round(float(in_query.double().mean()), 3)}), flush=True)
    for base in ("nearest", "rbf_sum"):
        print(json.dumps({"case": f"ratio_to_{base}", "rows": n,
                          **{name: round(res[name]["ms"] / res[base]["ms"], 4) for name in calls if name != base},
                          "largest_spread_pct": max(v["spread_pct"] for v in res.values())}), flush=True)


def prdc(n, repeats):
    val = BiologicalValidator({"evaluation": {}})
    real, synth = cohort(n, 3), cohort(n, 4)
    synth[: n // 2] = real[: n // 2] + 0.5 * synth[: n // 2]     # half of the synthetic rows near a real one, half on their own
    box = {}

    def run():
        box["res"] = val.fidelity_diversity(real, synth, k=5)

    run()
    runs = [clock(run) for _ in range(repeats)]
    print(json.dumps({"case": "prdc", "rows_per_cohort": n, "D": D, **stats(runs), **box["res"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16384,125000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prdc-sizes", default="16384,125000", help="rows per cohort of the end-to-end metrics; empty skips them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prdc_bench measures on a GPU: none found")
    for n in [int(s) for s in args.sizes.split(",") if s]:
        rectangle(n, args.repeats)
    for n in [int(s) for s in args.prdc_sizes.split(",") if s]:
        prdc(n, args.repeats)


if __name__ == "__main__":
    main()
