"""Rate of the Cox partial-likelihood kernels behind the survival utility (osd_val_cox_eval, csrc/cox.hip) against the same
computation in torch on the same tensors in the same process, the one-read yardstick osd_val_glm_eval beside them, the concordance
kernel, and ``survival_utility`` end to end (one JSON line per measurement).

  cox_eval        DeviceKernels.cox_eval, rows x D: w to the device, the score pass, the scans, the gradient pass, the slab
                  reduction, loss and gradient to the host -- X is read TWICE
  torch_cox       eta = X @ w'; exp, cumsum and gathers in double over the same host-made order and tie groups; G = r @ X in fp32
                  through torch, with the standardisation folded into w' and G as the kernels fold it -- X is read twice
  glm_grad        DeviceKernels.glm_eval(K = 1) with a gradient: one read of X
  glm_predict     DeviceKernels.glm_eval(K = 1, grad=False, scores=True): one read of X, no column accumulation
  concordance     DeviceKernels.concordance on n rows: n^2 ordered pairs are visited
  survival        BiologicalValidator.survival_utility on planted cohorts

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the four kernel cases alternate so
that a drift of the machine hits all alike.  A line reports the median, min and max, the spread (max - min) / median and the
effective GB/s of X: rows x D x 4 bytes counted TWICE for cox_eval and torch_cox, once for the two GLM calls.  For the kernels' own
times run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/survival_bench.py [--sizes 125000x2000,3000x5142] [--repeats 7] [--pairs 125000] [--e2e 20000x2000]
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


def cohort(n, D, seed):
    """Features (a rank-4 factor model plus unit noise) and survival columns under proportional hazards in the first four
    features: event time ~ Exp(mean 800 exp(-eta)), censoring ~ Exp(mean 1600), the observed time on a 30-day grid."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(4, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(99))
    x = torch.randn(n, 4, device="cuda", generator=g) @ w + torch.randn(n, D, device="cuda", generator=g)
    eta = (x[:, :4] * torch.tensor([1.0, -1.0, 0.5, -0.5], device="cuda")).sum(1) / x[:, :4].std()
    t_event = -torch.log1p(-torch.rand(n, device="cuda", generator=g)) * 800.0 * torch.exp(-eta)
    t_cens = -torch.log1p(-torch.rand(n, device="cuda", generator=g)) * 1600.0
    time_ = torch.ceil(torch.minimum(t_event, t_cens) / 30.0).clamp_(min=1.0) * 30.0
    surv = torch.stack([time_, (t_event <= t_cens).float()], dim=1)
    return x.contiguous(), surv.double().cpu().numpy()


def parse_sizes(text):
    return [tuple(int(v) for v in s.split("x")) for s in text.split(",") if s]


def kernel(rows, D, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x, surv = cohort(rows, D, 1)
    g = torch.Generator(device="cuda").manual_seed(7)
    center, scale = x.mean(0), 1.0 / x.std(0)
    w = torch.randn(D, device="cuda", generator=g) / D ** 0.5
    W = torch.cat([w, torch.zeros(1, device="cuda")])[None, :]
    y = (torch.rand(rows, 1, device="cuda", generator=g) < 0.5).float()
    plan = k.cox_plan(surv[:, 0], surv[:, 1])
    # what the plan holds, for torch: the descending-time order, the tie groups and the flags, made once on the host
    order = np.argsort(-surv[:, 0], kind="stable")
    ts = surv[order, 0]
    new = np.concatenate([[True], ts[1:] != ts[:-1]])
    starts = np.nonzero(new)[0]
    gid = np.cumsum(new) - 1
    dev = lambda a: torch.as_tensor(a, device="cuda")
    order_d, gstart, gend = dev(order), dev(starts[gid]), dev(np.concatenate([starts[1:] - 1, [rows - 1]])[gid])
    ds = dev(surv[order, 1])

    def torch_cox():
        w1 = w * scale
        eta = x @ w1 - (w1 @ center)
        es = eta.double()[order_d]
        m = es.max()
        e = torch.exp(es - m)
        S = torch.cumsum(e, 0)[gend]
        loss = -(ds * (es - m - torch.log(S))).sum()
        c = torch.flip(torch.cumsum(torch.flip(ds / S, [0]), 0), [0])[gstart]
        r = torch.empty(rows, device="cuda")
        r[order_d] = (-ds + e * c).float()
        grad = (r @ x - r.sum() * center) * scale
        return loss.cpu(), grad.cpu()

    calls = {"cox_eval": lambda: k.cox_eval(x, center, scale, w, plan), "torch_cox": torch_cox,
             "glm_grad": lambda: k.glm_eval(x, center, scale, y, W, [U.LOGISTIC]),
             "glm_predict": lambda: k.glm_eval(x, center, scale, None, W, [U.LOGISTIC], grad=False, scores=True)}
    reads = {"cox_eval": 2, "torch_cox": 2, "glm_grad": 1, "glm_predict": 1}
    for fn in calls.values():
        fn()
    ours, theirs = calls["cox_eval"](), calls["torch_cox"]()
    rel = float(np.abs(ours[1] - theirs[1].double().numpy()).max() / np.abs(ours[1]).max())
    rel_loss = abs(ours[0] - float(theirs[0])) / abs(ours[0])
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    plan.close()
    x_bytes = 4.0 * rows * D
    res = {name: stats(v, reads[name] * x_bytes) for name, v in runs.items()}
    aligned = x.data_ptr() % 16 == 0 and D % 4 == 0
    for name, v in res.items():
        print(json.dumps({"case": name, "rows": rows, "D": D, "x_mb": round(x_bytes / 1e6, 1), "x_reads": reads[name],
                          **({"sixteen_byte_path": aligned} if name != "torch_cox" else {}), **v}), flush=True)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D,
                      "cox_eval_over_torch_cox_time": round(res["cox_eval"]["ms"] / res["torch_cox"]["ms"], 4),
                      "cox_eval_over_glm_grad_plus_predict_time": round(res["cox_eval"]["ms"] / (res["glm_grad"]["ms"] + res["glm_predict"]["ms"]), 4),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()),
                      "gradient_max_rel_difference": float(f"{rel:.3e}"), "loss_rel_difference": float(f"{rel_loss:.3e}")}), flush=True)


def pairs(n, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    g = torch.Generator(device="cuda").manual_seed(11)
    time_ = torch.ceil(-torch.log1p(-torch.rand(n, device="cuda", generator=g)) * 600.0 / 30.0).clamp_(min=1.0) * 30.0
    event = (torch.rand(n, device="cuda", generator=g) < 0.65).float()
    risk = torch.randn(n, device="cuda", generator=g)
    box = {}

    def fn():
        box["c"] = k.concordance(time_, event, risk)

    fn()
    runs = sorted(clock(fn) for _ in range(repeats))
    med = runs[len(runs) // 2]
    print(json.dumps({"case": "concordance", "n": n, **stats(runs), "ordered_pairs_per_s": float(f"{n * n / med:.4e}"),
                      "comparable_pairs": box["c"][0], "comparable_pairs_per_s": float(f"{box['c'][0] / med:.4e}")}), flush=True)


def end_to_end(rows, D, repeats):
    val = BiologicalValidator({"evaluation": {}})
    (train, s_train), (synth, s_synth), (test, s_test) = cohort(rows, D, 2), cohort(rows, D, 3), cohort(max(rows // 4, 100), D, 4)
    box = {}

    def survival():
        box["s"] = val.survival_utility(train, s_train, synth, s_synth, test, s_test)

    survival()
    runs = [clock(survival) for _ in range(repeats)]
    shown = {key: round(v, 4) for key, v in box["s"].items() if "cindex" in key or "cosine" in key}
    print(json.dumps({"case": "survival", "rows_per_cohort": rows, "D": D, **stats(runs), **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000,3000x5142", help="rows x D of the kernel measurements")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", default="125000", help="n of the concordance measurements; empty skips them")
    ap.add_argument("--e2e", default="20000x2000", help="rows x D of the end-to-end runs; empty skips them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("survival_bench measures on a GPU: none found")
    for rows, D in parse_sizes(args.sizes):
        kernel(rows, D, args.repeats)
    for (n,) in parse_sizes(args.pairs):
        pairs(n, args.repeats)
    for rows, D in parse_sizes(args.e2e):
        end_to_end(rows, D, max(args.repeats // 2, 2))


if __name__ == "__main__":
    main()
