"""Rate of the centred Gram kernel behind the correlation-structure metrics (osd_val_centered_gram, csrc/corr.hip) against two
yardsticks on the same GPU from the same build, then ``correlation_fidelity`` end to end (one JSON line per measurement).

  centered_gram   DeviceKernels.centered_gram, rows x D: centres to the device, (for an X that 16-byte staging cannot read in place)
                  the padded copy, the Gram kernel over the upper-triangular tiles, the slice reduction with its mirror
  torch_product   (X - mu).T @ (X - mu) in fp32 through torch: the centred copy, the full D x D product, an fp32 result -- what the
                  metric would cost with a vendor GEMM (and without double sums)
  nearest         osd_val_nearest, n x n at D = 2000 (tools/privacy_bench.py): the same fp32 MFMA at a friendlier shape (K = 2000
                  contiguous, square tiles, no double sums)
  fidelity        BiologicalValidator.correlation_fidelity on two rows x D cohorts, without and with ``frechet=True``

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); a size's centered_gram and
torch_product repeats alternate so that a drift of the machine hits both alike.  A line reports the median, min and max and the
spread (max - min) / median.  TFLOP/s of the two Gram cases counts the NECESSARY operations, 2 rows D (D + 128) / 2 (the tiles on or
above the diagonal), over the whole call; of nearest, 2 n^2 D.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/corr_bench.py [--sizes 125000x2000,3000x5142] [--repeats 5] [--nearest 16384] [--fidelity 125000x2000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402


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


def cohort(n, D, seed, mix=0.0):
    """A rank-4 factor model plus unit noise with a 0/1 block in front; ``mix`` couples the halves (a second, different cohort)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(4, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(99))
    x = torch.randn(n, 4, device="cuda", generator=g) @ w + torch.randn(n, D, device="cuda", generator=g)
    if mix:
        x[:, :D // 2] += mix * x[:, D - D // 2:]
    x[:, :50] = (x[:, :50] > 0.5).float()
    return x.contiguous()


def parse_sizes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def gram(rows, D, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x = cohort(rows, D, 1)
    mu = x.double().mean(0)
    c = mu.cpu().numpy()
    mu32 = mu.float()

    def product():
        z = x - mu32
        return z.T @ z

    calls = {"centered_gram": lambda: k.centered_gram(x, c), "torch_product": product}
    for fn in calls.values():
        fn()
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    flop = 2.0 * rows * D * (D + 128) / 2
    res = {name: stats(v, flop) for name, v in runs.items()}
    in_place = x.data_ptr() % 16 == 0 and D % 4 == 0
    for name, v in res.items():
        print(json.dumps({"case": name, "rows": rows, "D": D, "necessary_gflop": round(flop / 1e9, 1),
                          **({"staged_in_place": in_place} if name == "centered_gram" else {}), **v}), flush=True)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D,
                      "centered_gram_over_torch_product_time": round(res["centered_gram"]["ms"] / res["torch_product"]["ms"], 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values())}), flush=True)


def nearest(n, repeats):
    D = 2000
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    q, r = cohort(n, D, 2), cohort(n, D, 3)
    k.nearest(q, r)
    runs = [clock(lambda: k.nearest(q, r)) for _ in range(repeats)]
    print(json.dumps({"case": "nearest", "queries": n, "references": n, "D": D, **stats(runs, 2.0 * n * n * D)}), flush=True)


def fidelity(rows, D, repeats):
    val = BiologicalValidator({"evaluation": {}})
    real, synth = cohort(rows, D, 4), cohort(rows, D, 5, mix=0.3)
    blocks = {"mutations": 50, "rest": D - 50}
    for frechet in (False, True):
        box = {}

        def run():
            box["res"] = val.correlation_fidelity(real, synth, blocks=blocks, frechet=frechet)

        run()
        runs = [clock(run) for _ in range(repeats)]
        extra = {"frechet_distance": round(box["res"]["frechet_distance"], 4)} if frechet else {}
        print(json.dumps({"case": "fidelity", "rows_per_cohort": rows, "D": D, "frechet": frechet, **stats(runs),
                          "corr_mean_abs_diff": round(box["res"]["corr_mean_abs_diff"], 5), **extra}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000,3000x5142", help="rows x D of the Gram measurements")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--nearest", default="16384", help="n of the n x n nearest-record yardstick; empty skips it")
    ap.add_argument("--fidelity", default="125000x2000", help="rows x D of the end-to-end runs; empty skips them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corr_bench measures on a GPU: none found")
    for rows, D in parse_sizes(args.sizes):
        gram(rows, D, args.repeats)
    for n in [int(s) for s in args.nearest.split(",") if s]:
        nearest(n, args.repeats)
    for rows, D in parse_sizes(args.fidelity):
        fidelity(rows, D, args.repeats)


if __name__ == "__main__":
    main()
