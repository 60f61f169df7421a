"""Time of the GSEA permutation null (osd_val_gsea, csrc/gsea.hip) against what a user would otherwise write in torch, on the same
inputs in the same run, then ``enrichment_fidelity`` end to end (one JSON line per measurement).

  gsea            DeviceKernels.gsea at perm_chunk = 0 (the library's choice): ES+ and ES- of S sets under the identity and P
                  permutations, results on the host; the ranks by the LDS sort (the default)
  gsea_count      the same call with OSD_GSEA_RANKS=count: the ranks by counting over the keys staged in LDS
  phases          either call's device milliseconds per phase (osd_val_gsea_timed: events around keys + ranks, the hit sort and the
                  scan, summed over the chunks) and the scan's share
  torch           the same definition composed on the device: a stable argsort of the SAME Philox keys (made beforehand, outside the
                  clock), its inverse by scatter, then per set a gather of the members' ranks, a sort, the weights' cumsum in float64,
                  the two ratios, max and min -- 1024 permutations at a time; the largest |difference| to the kernel's values
  fidelity        BiologicalValidator.enrichment_fidelity with one binary contrast on two cohorts of --rows patients

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the cases alternate so that a drift
of the machine hits all alike.  A line reports the median, min and max and the spread (max - min) / median.  The sets are drawn
without replacement from the D positions (the first five from the first D / 10, the columns the end-to-end cohorts shift in their
cases), sizes uniform in [15, 200]; the weights are |standard normal| values, sorted descending.

    python tools/gsea_bench.py [--shapes 5054x50x1000,5054x50x10000,20000x300x1000] [--repeats 5] [--rows 3000]
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402

PHASES = ("ranks", "hit_sort", "scan")
TAG_GSEA = 0x47534500
MASK = 0xFFFFFFFF


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


def philox_keys(seed, p0, p1, D):
    """int64 [p1 - p0, D] on the device: word 0 of Philox4x32-10 at counter (i, p, 0, TAG_GSEA), in int64 arithmetic (a product of two
    32-bit values wraps like the unsigned one; the high word is shifted down and masked)."""
    c0 = torch.arange(D, device="cuda", dtype=torch.int64)[None, :].expand(p1 - p0, D).clone()
    c1 = torch.arange(p0, p1, device="cuda", dtype=torch.int64)[:, None].expand(p1 - p0, D).clone()
    c2, c3 = torch.zeros_like(c0), torch.full_like(c0, TAG_GSEA)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        q0, q1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        hi0, lo0, hi1, lo1 = (q0 >> 32) & MASK, q0 & MASK, (q1 >> 32) & MASK, q1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0


def torch_gsea(w, sets, keys, D, rows=1024):
    """(es_pos, es_neg) float64 [P + 1, S] on the device by torch ops alone; keys int64 [P, D]."""
    P = keys.shape[0]
    pos_out, neg_out = [], []
    ident = torch.arange(D, device="cuda")[None, :]
    for p0 in [None] + list(range(0, P, rows)):                 # the identity first
        if p0 is None:
            rho = ident
        else:
            order = torch.argsort(keys[p0:p0 + rows], dim=1, stable=True)
            rho = torch.empty_like(order).scatter_(1, order, ident.expand_as(order))
        ep, en = [], []
        for m in sets:
            k = m.shape[0]
            h = rho[:, m].sort(dim=1).values
            c = w[h].cumsum(dim=1)
            nr = c[:, -1:]
            prev = torch.cat([torch.zeros_like(nr), c[:, :-1]], dim=1)
            miss = (h - torch.arange(k, device="cuda")[None, :]).double() / float(D - k)
            ep.append((c / nr - miss).max(dim=1).values)
            en.append((prev / nr - miss).min(dim=1).values)
        pos_out.append(torch.stack(ep, dim=1))
        neg_out.append(torch.stack(en, dim=1))
    return torch.cat(pos_out), torch.cat(neg_out)


def cohort(n, D, seed, shift):
    """(x fp32 [n, D] on the device, condition float64 [n] on the host): zero-inflated gamma values; the cases' first D / 10 columns
    are shifted."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand((3, n, D), device="cuda", generator=g)
    x = -1.5 * (torch.log1p(-u[0]) + torch.log1p(-u[1]))
    labels = (torch.rand(n, device="cuda", generator=g) < 0.4)
    x[:, :D // 10] += shift * labels[:, None]
    x = torch.where(u[2] < 0.3, torch.zeros_like(x), x)
    return x.contiguous(), labels.cpu().numpy().astype(np.float64)


def parse_shapes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def run(D, S, P, repeats, rows, seed=7):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    rs = np.random.default_rng(D + S)
    w = np.sort(np.abs(rs.standard_normal(D)))[::-1].copy()
    sets = [rs.choice(D // 10 if s < 5 else D, int(size), replace=False) for s, size in enumerate(rs.integers(15, 201, S))]
    shape = {"D": D, "sets": S, "members": int(sum(len(m) for m in sets)), "used_positions": int(np.unique(np.concatenate(sets)).size),
             "permutations": P}
    wd, sd = torch.from_numpy(w).cuda(), [torch.from_numpy(m).cuda() for m in sets]
    keys = torch.cat([philox_keys(seed, p0, min(p0 + 1024, P + 1), D) for p0 in range(1, P + 1, 1024)])
    box = {}

    def ours(mode):
        def call():
            os.environ["OSD_GSEA_RANKS"] = mode
            box[mode] = k.gsea(w, sets, P, seed)
        return call

    def composed():
        box["t"] = torch_gsea(wd, sd, keys, D)

    calls = {"gsea": ours("sort"), "gsea_count": ours("count"), "torch": composed}
    for fn in calls.values():
        fn()
    same = all(np.array_equal(box["sort"][f].view(np.int64), box["count"][f].view(np.int64)) for f in ("es_pos", "es_neg"))
    diff = max(float(np.abs(box["sort"][f] - t.cpu().numpy()).max()) for f, t in zip(("es_pos", "es_neg"), box["t"]))
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    res = {name: stats(v) for name, v in runs.items()}
    for name, v in res.items():
        print(json.dumps({"case": name, **shape, **v}), flush=True)
    print(json.dumps({"case": "ratio", **shape, "gsea_over_torch_time": round(res["gsea"]["ms"] / res["torch"]["ms"], 4),
                      "gsea_count_over_gsea_time": round(res["gsea_count"]["ms"] / res["gsea"]["ms"], 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()), "rank_kernels_same_bits": same,
                      "max_abs_difference_to_torch": float(f"{diff:.3e}")}), flush=True)
    for mode in ("sort", "count"):
        os.environ["OSD_GSEA_RANKS"] = mode
        med = np.median(np.array([k.gsea(w, sets, P, seed, phases=True)["phase_ms"] for _ in range(repeats)]), axis=0)
        print(json.dumps({"case": "phases", "ranks_by": mode, **shape, **{f"{name}_ms": round(float(med[i]), 3) for i, name in enumerate(PHASES)},
                          "device_ms": round(float(med.sum()), 3), "scan_share": round(float(med[2] / med.sum()), 3),
                          "dominant": PHASES[int(np.argmax(med))]}), flush=True)
    os.environ.pop("OSD_GSEA_RANKS", None)

    (x, cr), (y, cs) = cohort(rows, D, 1, 0.8), cohort(rows, D, 2, 0.8)
    val = BiologicalValidator({"evaluation": {}})
    named = {f"set{s}": m for s, m in enumerate(sets)}

    def fidelity():
        box["f"] = val.enrichment_fidelity(x, cr, y, cs, named, names=["group"], permutations=P, seed=seed)

    fidelity()
    v = stats([clock(fidelity) for _ in range(max(repeats // 2, 3))])
    shown = {key: round(float(box["f"][key]), 5) for key in ("gsea_nes_pearson_group", "gsea_real_hits_group", "gsea_recall_group")}
    print(json.dumps({"case": "fidelity", **shape, "rows": rows, **v, **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5054x50x1000,5054x50x10000,20000x300x1000", help="D x sets x permutations of each run")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=3000, help="patients per cohort of the end-to-end run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gsea_bench measures on a GPU: none found")
    for D, S, P in parse_shapes(args.shapes):
        run(D, S, P, args.repeats, args.rows)


if __name__ == "__main__":
    main()
