"""Time of the per-feature two-group rank statistics (osd_val_group_ranks, csrc/diffexp.hip) against the project's own two-cohort call on
the same rows split the same way and against what a user would otherwise write in torch, on the same tensors in the same run, then
``differential_fidelity`` end to end (one JSON line per measurement).

  group_ranks     DeviceKernels.group_ranks at chunk_cols = 0 (the library's choice): u2, ties and both groups' moments of all D
                  columns, results on the host
  phases          the same call's device milliseconds per phase (osd_val_group_ranks_timed: events around the label-partitioned
                  gather, the segmented sort and the statistics pass, summed over the chunks), and each phase's rate over the bytes
                  the algorithm moves per key (4-byte value of either group): gather 4 read + 4 written; sort 4 passes x (4 counted +
                  4 read again + 4 scattered) = 48; statistics 4 read once (its searches hit what the run just read)
  marginals       DeviceKernels.marginals on the case rows against the control rows, copied out beforehand: the same gather volume
                  and the same sort, then marg_stats where group_ranks runs de_stats -- the yardstick for the statistics pass; its
                  phases too
  torch           the two groups sorted (dim = 0), one searchsorted with right=False and one with right=True of the cases in the
                  controls for u2, the pooled column sorted and searched in itself for the tie sum (sum over the elements of
                  t^2 - 1), masked double sums for the moments, 256 columns at a time so that its temporaries stay within a few GB
  fidelity        BiologicalValidator.differential_fidelity with one binary contrast: two group_ranks calls plus the finite checks,
                  the column means and the summary

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the cases alternate so that a drift
of the machine hits all alike.  A line reports the median, min and max and the spread (max - min) / median.  The data are
zero-inflated and right-skewed like expression values (30 % exact zeros, a gamma tail); 40 % of the rows are cases, whose values
are scaled by 1.1.

    python tools/diffexp_bench.py [--sizes 125000x2000,3000x5142] [--repeats 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import _lib as L  # noqa: E402
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402

PHASES = ("gather", "sort", "statistics")
BYTES_PER_KEY = {"gather": 8, "sort": 48, "statistics": 4}


def stats(runs):
    runs = sorted(runs)
    med = runs[len(runs) // 2]
    return {"ms": round(1e3 * med, 3), "ms_min": round(1e3 * runs[0], 3), "ms_max": round(1e3 * runs[-1], 3),
            "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2), "repeats": len(runs)}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cohort(n, D, seed):
    """(x fp32 [n, D], labels int32 [n]) on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand((3, n, D), device="cuda", generator=g)
    x = -1.5 * (torch.log1p(-u[0]) + torch.log1p(-u[1]))          # gamma(2, 1.5)
    labels = (torch.rand(n, device="cuda", generator=g) < 0.4).to(torch.int32)
    x = torch.where(u[2] < 0.3, torch.zeros_like(x), x) * torch.where(labels == 1, 1.1, 1.0)[:, None]
    return x.contiguous(), labels


def torch_group_ranks(x, labels, center, cols=256):
    """(u2, ties int64 [D], sum, sumsq float64 [2, D]) by torch ops alone."""
    case, ctrl = labels == 1, labels == 0
    u2, ties, s, q = [], [], [], []
    for c0 in range(0, x.shape[1], cols):
        xc = x[:, c0:c0 + cols]
        a = xc[case].sort(dim=0).values.T.contiguous()
        b = xc[ctrl].sort(dim=0).values.T.contiguous()
        u2.append((torch.searchsorted(b, a, right=False) + torch.searchsorted(b, a, right=True)).sum(dim=1))
        pooled = torch.cat([a, b], dim=1).sort(dim=1).values
        t = torch.searchsorted(pooled, pooled, right=True) - torch.searchsorted(pooled, pooled, right=False)
        ties.append((t * t - 1).sum(dim=1))
        da, db = a.double() - center[c0:c0 + cols, None].double(), b.double() - center[c0:c0 + cols, None].double()
        s.append(torch.stack([da.sum(dim=1), db.sum(dim=1)]))
        q.append(torch.stack([(da * da).sum(dim=1), (db * db).sum(dim=1)]))
    return torch.cat(u2), torch.cat(ties), torch.cat(s, dim=1), torch.cat(q, dim=1)


def parse_sizes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def run(n, D, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x, labels = cohort(n, D, 1)
    center = x.mean(dim=0)
    cases, controls = x[labels == 1].contiguous(), x[labels == 0].contiguous()
    na, nb = int(cases.shape[0]), int(controls.shape[0])
    keys = float(na + nb) * D
    auto = L.lib().osd_val_marginals_auto_chunk(na, nb, D)
    shape = {"rows": n, "na": na, "nb": nb, "D": D, "mkeys": round(keys / 1e6, 1)}
    box = {}

    def ours():
        box["o"] = k.group_ranks(x, labels, center)

    def yardstick():
        box["m"] = k.marginals(cases, controls)

    def composed():
        box["t"] = torch_group_ranks(x, labels, center)

    calls = {"group_ranks": ours, "marginals": yardstick, "torch": composed}
    for fn in calls.values():
        fn()
    t_u2, t_ties, t_s, t_q = (v.cpu().numpy() for v in box["t"])
    same = bool(np.array_equal(box["o"]["u2"], t_u2) and np.array_equal(box["o"]["ties"], t_ties))
    mom_rel = float(max(np.max(np.abs(box["o"]["sum"] - t_s) / np.maximum(np.abs(t_s), 1e-300)),
                        np.max(np.abs(box["o"]["sumsq"] - t_q) / np.maximum(np.abs(t_q), 1e-300))))
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    res = {name: stats(v) for name, v in runs.items()}
    for name, v in res.items():
        extra = {"chunk_cols": auto, "algorithmic_gb_per_s": round(sum(BYTES_PER_KEY.values()) * keys / v["ms"] / 1e6, 1)} if name != "torch" else {}
        print(json.dumps({"case": name, **shape, **v, **extra}), flush=True)
    print(json.dumps({"case": "ratio", **shape, "group_ranks_over_marginals_time": round(res["group_ranks"]["ms"] / res["marginals"]["ms"], 4),
                      "group_ranks_over_torch_time": round(res["group_ranks"]["ms"] / res["torch"]["ms"], 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()), "integers_equal_torch": same,
                      "moments_max_relative_difference_to_torch": float(f"{mom_rel:.3e}")}), flush=True)

    for case, fn in (("phases", lambda: k.group_ranks(x, labels, center, phases=True)),
                     ("marginals_phases", lambda: k.marginals(cases, controls, phases=True))):
        med = np.median(np.array([fn()["phase_ms"] for _ in range(repeats)]), axis=0)
        print(json.dumps({"case": case, **shape, "chunk_cols": auto,
                          **{f"{name}_ms": round(float(med[i]), 3) for i, name in enumerate(PHASES)},
                          **{f"{name}_gb_per_s": round(BYTES_PER_KEY[name] * keys / float(med[i]) / 1e6, 1) for i, name in enumerate(PHASES)},
                          "device_ms": round(float(med.sum()), 3), "dominant": PHASES[int(np.argmax(med))]}), flush=True)

    y, y_labels = cohort(n, D, 2)
    val = BiologicalValidator({"evaluation": {}})
    cr, cs = labels.cpu().numpy().astype(np.float64), y_labels.cpu().numpy().astype(np.float64)

    def fidelity():
        box["f"] = val.differential_fidelity(x, cr, y, cs, names=["group"])

    fidelity()
    v = stats([clock(fidelity) for _ in range(max(repeats // 2, 3))])
    shown = {key: round(float(box["f"][key]), 5) for key in ("de_effect_pearson_group", "de_effect_slope_group", "de_recall_group",
                                                              "de_real_hits_group", "de_max_abs_effect_gap_group")}
    print(json.dumps({"case": "fidelity", **shape, **v, **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000,3000x5142", help="rows x D of each run")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffexp_bench measures on a GPU: none found")
    for n, D in parse_sizes(args.sizes):
        run(n, D, args.repeats)


if __name__ == "__main__":
    main()
