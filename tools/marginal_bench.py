"""Time of the all-feature marginal report (osd_val_marginals, csrc/marginal.hip) against the project's own KS-only path at full width
and against what a user would otherwise write in torch, on the same tensors in the same run, then the sweep over chunk_cols and
``marginal_fidelity`` end to end (one JSON line per measurement).

  marginals       DeviceKernels.marginals at chunk_cols = 0 (the library's choice): KS extremes, W1 and the range counts of all D
                  columns, results on the host
  phases          the same call's device milliseconds per phase (osd_val_marginals_timed: events around the transposing gather, the
                  segmented sort and the statistics pass, summed over the chunks), and each phase's rate over the bytes the
                  algorithm moves per key (4-byte value of either cohort): gather 4 read + 4 written; sort 4 passes x (4 counted +
                  4 read again + 4 scattered) = 48; statistics 4 read once (its searches and partners hit what the run just read)
  ks_extremes     DeviceKernels.ks_extremes with nf = D: the 100-column path of statistical_tests at full width -- KS only
  torch           sort(dim=0) of both cohorts, searchsorted of the pooled values in both for the KS extremes, and the coupling sum
                  for W1 with the (i, j, w) index arrays made beforehand, 256 columns at a time so that its temporaries stay
                  within a few GB
  chunk_sweep     marginals at each chunk_cols of --chunks (0 = auto)
  fidelity        BiologicalValidator.marginal_fidelity: the call above plus the finite checks, the column moments and the summary

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the cases alternate so that a drift
of the machine hits all alike.  A line reports the median, min and max and the spread (max - min) / median.  The data are
zero-inflated and right-skewed like expression values (30 % exact zeros, a gamma tail), the synthetic cohort slightly off.

    python tools/marginal_bench.py [--sizes 125000x125000x2000,100x3000x5142] [--repeats 5] [--chunks 0,8,16,32,64,128,256,512,1024,2048]
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


def cohort(n, D, seed, scale):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand((3, n, D), device="cuda", generator=g)
    x = -scale * (torch.log1p(-u[0]) + torch.log1p(-u[1]))          # gamma(2, scale)
    return torch.where(u[2] < 0.3, torch.zeros_like(x), x).contiguous()


def coupling(n1, n2):
    cuts = np.union1d(np.arange(n1, dtype=np.int64) * n2, np.arange(n2, dtype=np.int64) * n1)
    w = np.diff(np.append(cuts, np.int64(n1) * np.int64(n2)))
    return cuts // n2, cuts // n1, w


def torch_marginals(real, synth, pairs, cols=256):
    """(dmax, dmin int64 [D], w1 float64 [D]) by torch ops alone."""
    n1, n2, D = real.shape[0], synth.shape[0], real.shape[1]
    i, j, w = pairs
    dmax, dmin, w1 = [], [], []
    for c0 in range(0, D, cols):
        a = real[:, c0:c0 + cols].sort(dim=0).values.T.contiguous()
        b = synth[:, c0:c0 + cols].sort(dim=0).values.T.contiguous()
        pooled = torch.cat([a, b], dim=1)
        d = torch.searchsorted(a, pooled, right=True) * n2 - torch.searchsorted(b, pooled, right=True) * n1
        dmax.append(d.max(dim=1).values)
        dmin.append(d.min(dim=1).values)
        w1.append(((a[:, i].double() - b[:, j].double()).abs() * w).sum(dim=1) / (float(n1) * float(n2)))
    return torch.cat(dmax), torch.cat(dmin), torch.cat(w1)


def parse_sizes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def run(n1, n2, D, repeats, chunks):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    real, synth = cohort(n1, D, 1, 1.5), cohort(n2, D, 2, 1.6)
    pairs = tuple(torch.as_tensor(v, device="cuda") for v in coupling(n1, n2))
    pairs = (pairs[0], pairs[1], pairs[2].double())
    keys = float(n1 + n2) * D
    auto = L.lib().osd_val_marginals_auto_chunk(n1, n2, D)
    shape = {"n1": n1, "n2": n2, "D": D, "mkeys": round(keys / 1e6, 1)}
    box = {}

    def ours():
        box["o"] = k.marginals(real, synth)

    def ks_only():
        box["k"] = k.ks_extremes(real, synth, D)

    def composed():
        box["t"] = torch_marginals(real, synth, pairs)

    calls = {"marginals": ours, "ks_extremes": ks_only, "torch": composed}
    for fn in calls.values():
        fn()
    same_ks = bool(np.array_equal(box["o"]["ks_dmax"], box["k"][0]) and np.array_equal(box["o"]["ks_dmin"], box["k"][1])
                   and np.array_equal(box["o"]["ks_dmax"], box["t"][0].cpu().numpy()) and np.array_equal(box["o"]["ks_dmin"], box["t"][1].cpu().numpy()))
    w1_t = box["t"][2].cpu().numpy()
    w1_rel = float(np.max(np.abs(box["o"]["w1"] - w1_t) / np.maximum(w1_t, 1e-300)))
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    res = {name: stats(v) for name, v in runs.items()}
    for name, v in res.items():
        extra = {"chunk_cols": auto, "algorithmic_gb_per_s": round(sum(BYTES_PER_KEY.values()) * keys / v["ms"] / 1e6, 1)} if name == "marginals" else {}
        print(json.dumps({"case": name, **shape, **v, **extra}), flush=True)
    print(json.dumps({"case": "ratio", **shape, "marginals_over_ks_extremes_time": round(res["marginals"]["ms"] / res["ks_extremes"]["ms"], 4),
                      "marginals_over_torch_time": round(res["marginals"]["ms"] / res["torch"]["ms"], 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()), "ks_extremes_equal": same_ks,
                      "w1_max_relative_difference_to_torch": float(f"{w1_rel:.3e}")}), flush=True)

    ph = np.array([k.marginals(real, synth, phases=True)["phase_ms"] for _ in range(repeats)])
    med = np.median(ph, axis=0)
    print(json.dumps({"case": "phases", **shape, "chunk_cols": auto,
                      **{f"{name}_ms": round(float(med[i]), 3) for i, name in enumerate(PHASES)},
                      **{f"{name}_gb_per_s": round(BYTES_PER_KEY[name] * keys / float(med[i]) / 1e6, 1) for i, name in enumerate(PHASES)},
                      "device_ms": round(float(med.sum()), 3)}), flush=True)

    sweep = {c: [] for c in chunks if c <= D}
    for c in sweep:
        k.marginals(real, synth, chunk_cols=c)
    for _ in range(max(repeats // 2, 3)):
        for c in sweep:
            sweep[c].append(clock(lambda: k.marginals(real, synth, chunk_cols=c)))
    for c, v in sweep.items():
        cols = c if c else auto
        print(json.dumps({"case": "chunk_sweep", **shape, "chunk_cols": c, "columns_per_chunk": cols,
                          "buffers_mb": round(8.0 * (n1 + n2) * cols / 2 ** 20, 1), **stats(v)}), flush=True)

    val = BiologicalValidator({"evaluation": {}})

    def fidelity():
        box["f"] = val.marginal_fidelity(real, synth)

    fidelity()
    v = stats([clock(fidelity) for _ in range(max(repeats // 2, 3))])
    shown = {key: round(float(box["f"][key]), 5) for key in ("marginal_ks_mean", "marginal_ks_max", "marginal_w1_scaled_mean",
                                                              "marginal_w1_scaled_max", "marginal_out_of_range_share")}
    print(json.dumps({"case": "fidelity", **shape, **v, **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x125000x2000,100x3000x5142", help="n1 x n2 x D of each run")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunks", default="0,8,16,32,64,128,256,512,1024,2048", help="chunk_cols of the sweep (0: auto)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("marginal_bench measures on a GPU: none found")
    chunks = [int(v) for v in args.chunks.split(",") if v]
    for n1, n2, D in parse_sizes(args.sizes):
        run(n1, n2, D, args.repeats, chunks)


if __name__ == "__main__":
    main()
