"""Rate of the univariate Cox screen kernel (osd_val_cox_score, csrc/cox_score.hip) against its yardsticks on the same tensors in
the same process, and ``prognostic_fidelity`` end to end (one JSON line per measurement).

  cox_score_0     DeviceKernels.cox_score at beta = 0 (no exp), absmax wanted: the screen's first call -- X is read TWICE
  cox_score_beta  DeviceKernels.cox_score at beta uniform in [-1, 1] with the bound: a Newton iteration -- X is read twice, and
                  every element pays a double-precision exp in each read
  cox_eval_w0     DeviceKernels.cox_eval at w = 0 on the same plan: the existing two-read call, fp32 arithmetic on the X passes
  copy            a device copy of X: one read and one write
  torch_score     the same definition in torch: the rows gathered in time order once per call, then per chunk of columns float64
                  u, exp, three cumsums read at the tie groups' ends, and the sums over the events; values compared with ours
  prognostic      BiologicalValidator.prognostic_fidelity on two planted cohorts, with and without ``mle``

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the kernel cases alternate so that a
drift of the machine hits all alike.  A line reports the median, min and max, the spread (max - min) / median and the effective GB/s
of X: rows x D x 4 bytes counted twice for every case (for the copy: once read, once written).  For the kernels' own times run it
under `rocprofv3 --kernel-trace --stats -- python ...`.

    python tools/prognostic_bench.py [--sizes 125000x2000,3000x5142] [--repeats 7] [--e2e 125000x2000,3000x5142] [--chunk 250]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402
from survival_bench import clock, cohort, parse_sizes, stats  # noqa: E402


def kernel(rows, D, repeats, chunk):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x, surv = cohort(rows, D, 1)
    center, scale = x.mean(0), 1.0 / x.std(0)
    plan = k.cox_plan(surv[:, 0], surv[:, 1])
    _, _, _, absmax = k.cox_score(x, center, scale, plan, absmax=True)
    beta = torch.rand(D, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 2.0 - 1.0
    bound = torch.as_tensor(absmax, device="cuda")
    w0 = torch.zeros(D, device="cuda")
    sink = torch.empty_like(x)
    # what the plan holds, for torch: the descending-time order, the tie groups' ends and the flags, made once on the host
    order = np.argsort(-surv[:, 0], kind="stable")
    ts = surv[order, 0]
    starts = np.nonzero(np.concatenate([[True], ts[1:] != ts[:-1]]))[0]
    gid = np.cumsum(np.concatenate([[True], ts[1:] != ts[:-1]])) - 1
    dev = lambda a: torch.as_tensor(a, device="cuda")
    order_d, gend, ds = dev(order), dev(np.concatenate([starts[1:] - 1, [rows - 1]])[gid]), dev(surv[order, 1])[:, None]
    c64, s64 = center.double(), scale.double()

    def torch_score():
        xo = x[order_d]
        out = torch.empty((3, D), dtype=torch.float64, device="cuda")
        for lo in range(0, D, chunk):
            hi = min(D, lo + chunk)
            u = (xo[:, lo:hi].double() - c64[lo:hi]) * s64[lo:hi]
            arg = beta[lo:hi] * u - beta[lo:hi].abs() * bound[lo:hi]
            e = torch.exp(arg)
            eu = e * u
            a0 = torch.cumsum(e, 0)[gend]
            m1 = torch.cumsum(eu, 0)[gend] / a0
            m2 = torch.cumsum(eu * u, 0)[gend] / a0
            out[0, lo:hi] = (ds * (arg - torch.log(a0))).sum(0)
            out[1, lo:hi] = (ds * (u - m1)).sum(0)
            out[2, lo:hi] = (ds * (m2 - m1 * m1)).sum(0)
        return out.cpu().numpy()

    calls = {"cox_score_0": lambda: k.cox_score(x, center, scale, plan, absmax=True),
             "cox_score_beta": lambda: k.cox_score(x, center, scale, plan, beta=beta, bound=bound),
             "cox_eval_w0": lambda: k.cox_eval(x, center, scale, w0, plan),
             "copy": lambda: sink.copy_(x),
             "torch_score": torch_score}
    for fn in calls.values():
        fn()
    ours, theirs = calls["cox_score_beta"](), calls["torch_score"]()
    rel = [float(np.abs(ours[i] - theirs[i]).max() / np.abs(ours[i]).max()) for i in range(3)]
    zero, grad = calls["cox_score_0"](), calls["cox_eval_w0"]()[1]
    rel_grad = float(np.abs(zero[1] + grad).max() / np.abs(grad).max())
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    plan.close()
    x_bytes = 4.0 * rows * D
    res = {name: stats(v, 2 * x_bytes) for name, v in runs.items()}
    aligned = x.data_ptr() % 16 == 0 and D % 4 == 0
    for name, v in res.items():
        print(json.dumps({"case": name, "rows": rows, "D": D, "x_mb": round(x_bytes / 1e6, 1), "x_passes": 2,
                          **({"sixteen_byte_path": aligned} if name.startswith("cox_") else {}), **v}), flush=True)
    ratio = lambda a, b: round(res[a]["ms"] / res[b]["ms"], 4)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D, "cox_score_0_over_cox_eval_w0_time": ratio("cox_score_0", "cox_eval_w0"),
                      "cox_score_beta_over_cox_eval_w0_time": ratio("cox_score_beta", "cox_eval_w0"),
                      "cox_score_beta_over_cox_score_0_time": ratio("cox_score_beta", "cox_score_0"),
                      "cox_score_0_over_copy_time": ratio("cox_score_0", "copy"),
                      "cox_score_beta_over_torch_score_time": ratio("cox_score_beta", "torch_score"),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()),
                      "loglik_score_info_max_rel_difference_to_torch": [float(f"{v:.3e}") for v in rel],
                      "score_0_plus_cox_eval_gradient_max_rel": float(f"{rel_grad:.3e}")}), flush=True)


def end_to_end(rows, D, repeats):
    val = BiologicalValidator({"evaluation": {}})
    (real, s_real), (synth, s_synth) = cohort(rows, D, 2), cohort(rows, D, 3)
    for mle in (True, False):
        box = {}

        def prognostic():
            box["s"], box["rows"] = val.prognostic_fidelity(real, s_real, synth, s_synth, mle=mle, return_rows=True)

        prognostic()
        runs = [clock(prognostic) for _ in range(repeats)]
        shown = {key: (round(v, 4) if isinstance(v, float) else v) for key, v in box["s"].items()
                 if key in ("prog_effect_slope", "prog_effect_pearson", "prog_real_hits", "prog_synth_hits", "prog_recall",
                            "prog_not_converged_real", "prog_not_converged_synth")}
        calls = int(box["rows"]["real"]["iterations"].max()) + 1 if mle else 1
        print(json.dumps({"case": "prognostic", "mle": mle, "rows_per_cohort": rows, "D": D, "kernel_calls_per_cohort": calls,
                          **stats(runs), **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000,3000x5142", help="rows x D of the kernel measurements")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--e2e", default="125000x2000,3000x5142", help="rows x D of the end-to-end runs; empty skips them")
    ap.add_argument("--chunk", type=int, default=250, help="columns of one float64 chunk of the torch composition")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prognostic_bench measures on a GPU: none found")
    for rows, D in parse_sizes(args.sizes):
        kernel(rows, D, args.repeats, args.chunk)
    for rows, D in parse_sizes(args.e2e):
        end_to_end(rows, D, max(args.repeats // 2, 2))


if __name__ == "__main__":
    main()
