"""Time of per-patient pathway scoring (osd_val_pathway_scores, csrc/pathway.hip) against its floor and against what a user would
otherwise write in torch, on the same inputs in the same run (one JSON line per measurement).

  copy            a device-to-device copy of X: one read (and one write) of the matrix, the floor of the linear methods
  mean, zscore,   DeviceKernels.pathway_scores: S sets scored in every row of X, the float64 scores left on the device
  ssgsea
  torch_<method>  the same definition composed on the device, the genes some set uses gathered first.  Linear methods: the
                  differences and products in float64, then a dense float64 product with the genes x sets 0/1 matrix.  ssgsea, 8192 rows
                  at a time: a row-wise torch.sort, two searchsorted calls (left and right) for twice the mid-rank, a gather from the
                  SAME host-made table, then the three float64 products with the 0/1 matrix.  The largest |difference| to the
                  kernel's values is reported
  ssgsea_one_set  the ssgsea call with the first set alone: the row's load and sort with next to no searches or sums -- what is left of
                  ssgsea's time beyond it goes to the members' searches and the set sums (the kernel is one launch: events cannot
                  split it)
  phases          the kernel's device milliseconds per phase (osd_val_pathway_scores_timed: events around the staging of the tables
                  and around the scoring launches)

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the cases alternate so that a drift
of the machine hits all alike.  A line reports the median, min and max, the spread (max - min) / median and the rate at which X
(rows * D * 4 bytes) goes by.  Rows are zero-inflated (30 % zeros, a gamma tail); the sets are drawn without replacement from the D
genes, sizes uniform in [15, 200].

    python tools/pathway_bench.py [--shapes 3000x5054x50,125000x2000x50,100000x5054x50] [--repeats 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.pathways import rank_table  # noqa: E402
from osteosarcoma_diffusionmodel_amd.validation import DeviceKernels  # noqa: E402

METHODS = ("mean", "zscore", "ssgsea")
PHASES = ("staging", "scoring")
SORT_ROWS = 8192


def stats(runs, x_bytes):
    runs = sorted(runs)
    med = runs[len(runs) // 2]
    return {"ms": round(1e3 * med, 3), "ms_min": round(1e3 * runs[0], 3), "ms_max": round(1e3 * runs[-1], 3),
            "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2), "repeats": len(runs), "x_gb_per_s": round(x_bytes / med / 1e9, 1)}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cohort(n, D, seed):
    """x fp32 [n, D] on the device: zero-inflated gamma values, made 16384 rows at a time."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((n, D), dtype=torch.float32, device="cuda")
    for r0 in range(0, n, 16384):
        u = torch.rand((3, min(16384, n - r0), D), device="cuda", generator=g)
        v = -1.5 * (torch.log1p(-u[0]) + torch.log1p(-u[1]))
        x[r0:r0 + v.shape[0]] = torch.where(u[2] < 0.3, torch.zeros_like(v), v)
    return x


def torch_linear(x, used, member, norm, c, s):
    """float64 [rows, S]: ((x - c) s) over the used genes in float64, times the 0/1 matrix, over the norm."""
    d = x[:, used].double()
    if c is not None:
        d = (d - c) * s
    return (d @ member) / norm


def torch_ssgsea(x, used, member, sizes, table, D):
    """float64 [rows, S] by sort, two searchsorted calls, a table gather and three float64 products, SORT_ROWS rows at a time."""
    out = []
    for r0 in range(0, x.shape[0], SORT_ROWS):
        part = x[r0:r0 + SORT_ROWS]
        vals = torch.sort(part, dim=1).values
        xg = part[:, used].contiguous()
        r2 = torch.searchsorted(vals, xg, right=False) + torch.searchsorted(vals, xg, right=True) + 1
        t, r = table[r2], 0.5 * r2.double()
        out.append((r * t) @ member / (t @ member) - (D * (D + 1) / 2.0 - r @ member) / (D - sizes))
    return torch.cat(out)


def parse_shapes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def run(rows, D, S, repeats, seed=7):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    rs = np.random.default_rng(D + S)
    sets = [rs.choice(D, int(size), replace=False) for size in rs.integers(15, 201, S)]
    used_np = np.unique(np.concatenate(sets))
    shape = {"rows": rows, "D": D, "sets": S, "members": int(sum(len(m) for m in sets)), "used_genes": int(used_np.size)}
    x = cohort(rows, D, seed)
    x_bytes = rows * D * 4
    table_np = rank_table(D)
    center = x[: min(rows, 4096)].double().mean(dim=0).float()
    scale = (1.0 / x[: min(rows, 4096)].double().std(dim=0).clamp_min(1e-6)).float()
    args = {"mean": {}, "zscore": dict(center=center, scale=scale), "ssgsea": dict(rank_table=table_np)}
    # the torch side's tables
    used = torch.from_numpy(used_np).cuda()
    slot = {int(g): i for i, g in enumerate(used_np)}
    member_np = np.zeros((used_np.size, S))
    for q, m in enumerate(sets):
        member_np[[slot[int(g)] for g in m], q] = 1.0
    member = torch.from_numpy(member_np).cuda()
    sizes = torch.tensor([float(len(m)) for m in sets], dtype=torch.float64, device="cuda")
    table = torch.from_numpy(table_np).cuda()
    c64, s64 = center.double()[used], scale.double()[used]
    dst = torch.empty_like(x)
    box = {}

    def ours(method):
        def call():
            box[method] = k.pathway_scores(x, sets, method, **args[method])
        return call

    def composed(method):
        def call():
            if method == "ssgsea":
                box["torch_" + method] = torch_ssgsea(x, used, member, sizes, table, D)
            elif method == "mean":
                box["torch_" + method] = torch_linear(x, used, member, sizes, None, None)
            else:
                box["torch_" + method] = torch_linear(x, used, member, sizes.sqrt(), c64, s64)
        return call

    calls = {"copy": lambda: dst.copy_(x)}
    for method in METHODS:
        calls[method], calls["torch_" + method] = ours(method), composed(method)
    calls["ssgsea_one_set"] = lambda: k.pathway_scores(x, sets[:1], "ssgsea", rank_table=table_np)
    for fn in calls.values():
        fn()
    diff = {m: float((box[m] - box["torch_" + m]).abs().max()) for m in METHODS}
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    res = {name: stats(v, x_bytes) for name, v in runs.items()}
    for name, v in res.items():
        print(json.dumps({"case": name, **shape, **v}), flush=True)
    for m in METHODS:
        print(json.dumps({"case": "ratio", "method": m, **shape, "kernel_over_torch_time": round(res[m]["ms"] / res["torch_" + m]["ms"], 4),
                          "kernel_over_copy_time": round(res[m]["ms"] / res["copy"]["ms"], 3),
                          "larger_spread_pct": max(res[m]["spread_pct"], res["torch_" + m]["spread_pct"]),
                          "max_abs_difference_to_torch": float(f"{diff[m]:.3e}")}), flush=True)
        med = np.median(np.array([k.pathway_scores(x, sets, m, phases=True, **args[m])[1] for _ in range(repeats)]), axis=0)
        print(json.dumps({"case": "phases", "method": m, **shape, **{f"{name}_ms": round(float(med[i]), 3) for i, name in enumerate(PHASES)},
                          "device_ms": round(float(med.sum()), 3), "host_and_sync_ms": round(res[m]["ms"] - float(med.sum()), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3000x5054x50,125000x2000x50,100000x5054x50", help="rows x D x sets of each run")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pathway_bench measures on a GPU: none found")
    for rows, D, S in parse_shapes(a.shapes):
        run(rows, D, S, a.repeats)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
