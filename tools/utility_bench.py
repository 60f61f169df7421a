"""Rate of the regularised-linear-model kernel behind the downstream-utility metrics (osd_val_glm_eval, csrc/glm.hip) against the
two-product formulation in torch on the same tensors in the same process, then ``downstream_utility`` and ``discriminator_test``
end to end (one JSON line per measurement).

  glm_eval        DeviceKernels.glm_eval, rows x D with K heads: W to the device, the one-pass kernel (dot, link function, column
                  accumulation over the same read of X), the slab reduction, loss and gradient to the host
  torch_products  Z = X @ W'.T; the residual; G = R.T @ X in fp32 through torch, with the standardisation folded into W' and G
                  as the kernel folds it -- what an iteration would cost with two vendor GEMMs: X is read twice
  utility / c2st  BiologicalValidator.downstream_utility (three conditions) and discriminator_test on planted cohorts

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); glm_eval and torch_products
alternate so that a drift of the machine hits both alike.  A line reports the median, min and max, the spread (max - min) / median
and the effective GB/s of X: rows x D x 4 bytes ONCE over the whole call, for both cases.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/utility_bench.py [--sizes 125000x2000x1,125000x2000x3,3000x5142x1,3000x5142x3] [--repeats 7] [--e2e 20000x2000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import utility as U  # noqa: E402
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


def cohort(n, D, seed, conditions=3):
    """Features (a rank-4 factor model plus unit noise) and conditions planted in the first columns: even ones binary with a
    logit linear in four features, odd ones continuous with a mean linear in four."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(4, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(99))
    x = torch.randn(n, 4, device="cuda", generator=g) @ w + torch.randn(n, D, device="cuda", generator=g)
    cond = torch.empty(n, conditions, device="cuda")
    for j in range(conditions):
        lin = (x[:, 4 * j:4 * j + 4] * torch.tensor([1.0, -1.0, 0.5, -0.5], device="cuda")).sum(1) / x[:, 4 * j:4 * j + 4].std()
        noise = torch.randn(n, device="cuda", generator=g)
        cond[:, j] = (torch.rand(n, device="cuda", generator=g) < torch.sigmoid(2.0 * lin)).float() if j % 2 == 0 else 300.0 + 100.0 * lin + 40.0 * noise
    return x.contiguous(), cond


def parse_sizes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def kernel(rows, D, K, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x, _ = cohort(rows, D, 1)
    g = torch.Generator(device="cuda").manual_seed(7)
    center, sd = x.mean(0), x.std(0)
    scale = 1.0 / sd
    kinds = [U.LOGISTIC if j % 2 == 0 else U.SQUARED for j in range(K)]
    y = (torch.rand(rows, K, device="cuda", generator=g) < 0.5).float()
    W = torch.randn(K, D + 1, device="cuda", generator=g) / D ** 0.5
    logistic = torch.tensor([v == U.LOGISTIC for v in kinds], device="cuda")

    def products():
        w1 = W[:, :D] * scale
        z = x @ w1.T + (W[:, D] - w1 @ center)
        r = torch.where(logistic, torch.sigmoid(z), z) - y
        loss = torch.where(logistic, torch.nn.functional.softplus(z) - y * z, 0.5 * (z - y) ** 2).sum(0)
        grad = (r.T @ x - r.sum(0)[:, None] * center) * scale
        return loss.cpu(), torch.cat([grad, r.sum(0)[:, None]], dim=1).cpu()

    calls = {"glm_eval": lambda: k.glm_eval(x, center, scale, y, W, kinds), "torch_products": products}
    ours, theirs = calls["glm_eval"](), calls["torch_products"]()
    rel = float(np.abs(ours[1] - theirs[1].double().numpy()).max() / np.abs(ours[1]).max())
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    x_bytes = 4.0 * rows * D
    res = {name: stats(v, x_bytes) for name, v in runs.items()}
    aligned = x.data_ptr() % 16 == 0 and D % 4 == 0
    for name, v in res.items():
        print(json.dumps({"case": name, "rows": rows, "D": D, "K": K, "x_mb": round(x_bytes / 1e6, 1),
                          **({"sixteen_byte_path": aligned} if name == "glm_eval" else {}), **v}), flush=True)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D, "K": K,
                      "glm_eval_over_torch_products_time": round(res["glm_eval"]["ms"] / res["torch_products"]["ms"], 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()),
                      "gradient_max_rel_difference": float(f"{rel:.3e}")}), flush=True)


def end_to_end(rows, D, repeats):
    val = BiologicalValidator({"evaluation": {}})
    (train, c_train), (synth, c_synth), (test, c_test) = cohort(rows, D, 2), cohort(rows, D, 3), cohort(max(rows // 4, 100), D, 4)
    names = ["event", "time", "metastasis"]
    box = {}

    def utility():
        box["u"] = val.downstream_utility(train, c_train, synth, c_synth, test, c_test, names=names)

    def c2st():
        box["c"] = val.discriminator_test(train, synth)

    for name, fn in (("utility", utility), ("c2st", c2st)):
        fn()
        runs = [clock(fn) for _ in range(repeats)]
        shown = {key: round(v, 4) for key, v in box[name[0]].items() if "gap" in key or key.startswith("c2st")}
        print(json.dumps({"case": name, "rows_per_cohort": rows, "D": D, **stats(runs), **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000x1,125000x2000x3,3000x5142x1,3000x5142x3", help="rows x D x K of the kernel measurements")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--e2e", default="20000x2000", help="rows x D of the end-to-end runs; empty skips them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("utility_bench measures on a GPU: none found")
    for rows, D, K in parse_sizes(args.sizes):
        kernel(rows, D, K, args.repeats)
    for rows, D in parse_sizes(args.e2e):
        end_to_end(rows, D, max(args.repeats // 2, 2))


if __name__ == "__main__":
    main()
