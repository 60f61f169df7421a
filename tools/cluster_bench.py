"""Rate of the label-sum kernel behind k-means and subtype fidelity (osd_val_label_sums, csrc/cluster.hip) against the project's own
one-pass stream over the same bytes and against what a user would otherwise write in torch, then one Lloyd iteration split into its
halves and ``subtype_fidelity`` end to end (one JSON line per measurement).

  label_sums      DeviceKernels.label_sums, rows x D with K labels: the kernel (per-label double accumulators in LDS, one slab per
                  row block), the slab reduction, the synchronise; results stay on the device
  col_moments     DeviceKernels.col_centered_moments on the same tensor: one pass over the same bytes, two double sums per column in
                  registers, results to the host -- the streaming yardstick
  torch_index_add float64 zeros [K, D] .index_add_(0, labels, x.double()): the same sums through torch (it converts X to double
                  first: 3 x the bytes of X written and read again)
  assign / update the halves of one Lloyd iteration: DeviceKernels.nearest against K centroids, and label_sums with the division
  subtype         BiologicalValidator.subtype_fidelity on planted cohorts

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the kernel cases alternate so that a
drift of the machine hits all alike.  A line reports the median, min and max, the spread (max - min) / median and the effective
GB/s of X: rows x D x 4 bytes ONCE over the whole call, for every case.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/cluster_bench.py [--sizes 125000x2000x8] [--repeats 7] [--e2e 125000x2000x8]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402


def stats(runs, x_bytes=None):
    runs = sorted(runs)
    med = runs[len(runs) // 2]
    out = {"ms": round(1e3 * med, 3), "ms_min": round(1e3 * runs[0], 3), "ms_max": round(1e3 * runs[-1], 3),
           "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2), "repeats": len(runs)}
    if x_bytes is not None:
        out["x_gb_per_s"] = round(x_bytes / med / 1e9, 1)
        out["x_gb_per_s_best"] = round(x_bytes / runs[0] / 1e9, 1)
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cohort(n, D, K, seed, weights=None):
    """K Gaussian blobs (centres 3 N(0, 1), unit noise), centred as subtype_fidelity centres its inputs."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mu = 3.0 * torch.randn(K, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(99))
    w = torch.ones(K, device="cuda") if weights is None else torch.as_tensor(weights, dtype=torch.float32, device="cuda")
    truth = torch.multinomial(w, n, replacement=True, generator=g)
    x = mu[truth] + torch.randn(n, D, device="cuda", generator=g)
    return (x - mu.mean(0)).contiguous(), truth


def parse_sizes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def kernel(rows, D, K, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x, _ = cohort(rows, D, K, 1)
    labels = torch.randint(0, K, (rows,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)).to(torch.int32)
    long_labels = labels.to(torch.int64)
    box = {}

    def index_add():
        box["t"] = torch.zeros((K, D), dtype=torch.float64, device="cuda").index_add_(0, long_labels, x.double())

    def ours():
        box["o"] = k.label_sums(x, labels, K)[0]

    calls = {"label_sums": ours, "col_moments": lambda: k.col_centered_moments(x), "torch_index_add": index_add}
    for fn in calls.values():
        fn()
    scale = float(torch.zeros((K, D), dtype=torch.float64, device="cuda").index_add_(0, long_labels, x.double().abs()).max())
    rel = float((box["o"] - box["t"]).abs().max()) / scale
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    x_bytes = 4.0 * rows * D
    res = {name: stats(v, x_bytes) for name, v in runs.items()}
    for name, v in res.items():
        print(json.dumps({"case": name, "rows": rows, "D": D, "K": K, "x_mb": round(x_bytes / 1e6, 1), **v}), flush=True)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D, "K": K,
                      "label_sums_over_col_moments_time": round(res["label_sums"]["ms"] / res["col_moments"]["ms"], 4),
                      "label_sums_over_torch_index_add_time": round(res["label_sums"]["ms"] / res["torch_index_add"]["ms"], 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()),
                      "sums_max_difference_over_sum_abs": float(f"{rel:.3e}")}), flush=True)

    # one Lloyd iteration from K rows of x: assignment, then update
    C = x[torch.randperm(rows, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))[:K]].contiguous()

    def assign():
        box["a"] = k.nearest(x, C)

    def update():
        sums, counts, _ = k.label_sums(x, box["a"][1], K)
        box["c"] = (sums / counts.clamp(min=1).double().unsqueeze(1)).float()

    assign(), update()
    halves = {"assign": [], "update": []}
    for _ in range(repeats):
        halves["assign"].append(clock(assign))
        halves["update"].append(clock(update))
    res = {name: stats(v, x_bytes) for name, v in halves.items()}
    for name, v in res.items():
        print(json.dumps({"case": f"lloyd_{name}", "rows": rows, "D": D, "K": K, **v}), flush=True)
    print(json.dumps({"case": "lloyd_iteration", "rows": rows, "D": D, "K": K, "ms": round(res["assign"]["ms"] + res["update"]["ms"], 3),
                      "update_share": round(res["update"]["ms"] / (res["assign"]["ms"] + res["update"]["ms"]), 4)}), flush=True)


def end_to_end(rows, D, K, repeats):
    val = BiologicalValidator({"evaluation": {}})
    weights = np.arange(K, 0, -1.0)
    (real, _), (synth, _) = cohort(rows, D, K, 2, weights), cohort(rows, D, K, 3, weights)
    box = {}

    def subtype():
        box["s"] = val.subtype_fidelity(real, synth, K)

    subtype()
    runs = [clock(subtype) for _ in range(repeats)]
    shown = {key: round(float(box["s"][key]), 5) for key in ("subtype_js_divergence", "subtype_tv_distance", "subtype_dispersion_ratio_min",
                                                              "subtype_centroid_shift_max", "subtype_iterations", "subtype_missing")}
    print(json.dumps({"case": "subtype", "rows_per_cohort": rows, "D": D, "K": K, **stats(runs), **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000x8", help="rows x D x K of the kernel measurements")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--e2e", default="125000x2000x8", help="rows x D x K of the end-to-end runs; empty skips them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench measures on a GPU: none found")
    for rows, D, K in parse_sizes(args.sizes):
        kernel(rows, D, K, args.repeats)
    for rows, D, K in parse_sizes(args.e2e):
        end_to_end(rows, D, K, max(args.repeats // 2, 2))


if __name__ == "__main__":
    main()
