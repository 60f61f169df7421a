"""Rate of the feature-transform kernel (osd_xf_apply, csrc/transform.hip) against the stream floor and against
the torch composition of the same map, then ``generate_scenarios`` end to end with and without a transform (one JSON line per
measurement).

  xf_forward / xf_inverse   FeatureTransform.forward / inverse on a dense rows x D matrix, every column quantile_normal with Q levels:
                            the kind read-back, the kernel (one read and one write of the matrix, the searches in LDS), a synchronise
  copy                      a device-to-device ``copy_`` of the same bytes: the stream floor, one read and one write
  torch_forward             the same map in torch: ``searchsorted`` left and right on the transposed copy against the [D, Q] knots,
                            gathers of the bracketing knots and levels, the lerp, the mid-rank and clamp selects, the transpose back
  torch_inverse             ``searchsorted`` of z in the shared levels, gathers from the transposed knots, the lerp, the clamp selects
  generate                  SyntheticPatientGenerator.generate_scenarios, 3 scenarios x 1000 patients at the reference's dimensions
                            (50 / 1900 / 50, hidden [256, 512, 256], T = 1000), with and without ``model.feature_transform``

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the cases of one shape alternate so
that a drift of the machine hits all alike.  A line reports the median, min and max, the spread (max - min) / median and the
effective GB/s: rows x D x 4 bytes read and as many written, ONCE, for every case.  The torch composition is also compared with the
kernel: the largest difference over the matrix is printed with the ratios.

    python tools/transform_bench.py [--sizes 100000x2000,100000x5142] [--levels 1000] [--repeats 7] [--generate 3x1000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, SyntheticPatientGenerator  # noqa: E402
from osteosarcoma_diffusionmodel_amd.transform import FeatureTransform  # noqa: E402


def stats(runs, nbytes=None):
    runs = sorted(runs)
    med = runs[len(runs) // 2]
    out = {"ms": round(1e3 * med, 3), "ms_min": round(1e3 * runs[0], 3), "ms_max": round(1e3 * runs[-1], 3),
           "spread_pct": round(100 * (runs[-1] - runs[0]) / med, 2), "repeats": len(runs)}
    if nbytes is not None:
        out["gb_per_s"] = round(nbytes / med / 1e9, 1)
        out["gb_per_s_best"] = round(nbytes / runs[0] / 1e9, 1)
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def cohort(n, D, seed):
    """Zero-inflated log-expression: about 30 % exact zeros per column, the rest log2(1 + a log-normal count)."""
    rs = np.random.default_rng(seed)
    counts = np.floor(np.exp(rs.normal(4.0, 2.0, (n, D))))
    counts[rs.random((n, D)) < 0.3] = 0.0
    return np.log2(counts + 1.0).astype(np.float32)


def torch_forward(x, knots, zl):
    Q = zl.shape[0]
    xt = x.t().contiguous()
    lb, ub = torch.searchsorted(knots, xt, right=False), torch.searchsorted(knots, xt, right=True)
    j = (lb - 1).clamp(0, Q - 2)
    k0, k1 = knots.gather(1, j), knots.gather(1, j + 1)
    z0, z1 = zl[j], zl[j + 1]
    out = z0 + (xt - k0) / (k1 - k0) * (z1 - z0)
    s = lb + ub
    mid = 0.5 * (zl[((s - 1) >> 1).clamp(0, Q - 1)] + zl[(s >> 1).clamp(0, Q - 1)])
    out = torch.where(ub > lb, mid, out)
    out = torch.where(ub == 0, zl[0], out)
    out = torch.where(lb == Q, zl[Q - 1], out)
    out = torch.where(torch.isnan(xt), xt, out)
    return out.t().contiguous()


def torch_inverse(z, knots_t, zl):
    Q = zl.shape[0]
    j = (torch.searchsorted(zl, z, right=True) - 1).clamp(0, Q - 2)
    k0, k1 = knots_t.gather(0, j), knots_t.gather(0, j + 1)
    z0, z1 = zl[j], zl[j + 1]
    out = k0 + (z - z0) / (z1 - z0) * (k1 - k0)
    out = torch.where(z <= zl[0], knots_t[0].expand_as(z), out)
    out = torch.where(z >= zl[Q - 1], knots_t[Q - 1].expand_as(z), out)
    return torch.where(torch.isnan(z), z, out)


def kernel(rows, D, Q, repeats):
    blocks = {"mutations": 0, "expression": D, "pathways": 0}
    ft = FeatureTransform.fit(cohort(max(Q, 1000), D, 1), blocks, {"expression": "quantile_normal"}, n_quantiles=Q)
    g = torch.Generator(device="cuda").manual_seed(5)
    # data drawn from the fitted columns' own range: zeros on the plateau, the rest between the knots
    u = torch.rand(rows, D, device="cuda", generator=g)
    hi = ft.knots[:, -1].cuda()
    x = torch.where(u < 0.3, torch.zeros((), device="cuda"), u * hi).contiguous()
    z = torch.randn(rows, D, device="cuda", generator=g)
    knots, zl = ft.knots.cuda(), ft.levels.cuda()
    knots_t = knots.t().contiguous()
    out, box = torch.empty_like(x), {}

    def t_fwd():
        box["tf"] = torch_forward(x, knots, zl)

    def t_inv():
        box["ti"] = torch_inverse(z, knots_t, zl)

    calls = {"xf_forward": lambda: ft.forward(x, out=out), "xf_inverse": lambda: ft.inverse(z, out=out), "copy": lambda: out.copy_(x),
             "torch_forward": t_fwd, "torch_inverse": t_inv}
    for fn in calls.values():
        fn()
    diff_f = float((ft.forward(x) - box["tf"]).abs().max())
    diff_i = float((ft.inverse(z) - box["ti"]).abs().max())
    box.clear()
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
            box.clear()
    nbytes = 8.0 * rows * D
    res = {name: stats(v, nbytes) for name, v in runs.items()}
    for name, v in res.items():
        print(json.dumps({"case": name, "rows": rows, "D": D, "Q": int(zl.shape[0]), "mb_read_and_written": round(nbytes / 1e6, 1), **v}), flush=True)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D, "Q": int(zl.shape[0]),
                      "xf_forward_over_copy_time": round(res["xf_forward"]["ms"] / res["copy"]["ms"], 3),
                      "xf_inverse_over_copy_time": round(res["xf_inverse"]["ms"] / res["copy"]["ms"], 3),
                      "torch_forward_over_xf_forward_time": round(res["torch_forward"]["ms"] / res["xf_forward"]["ms"], 2),
                      "torch_inverse_over_xf_inverse_time": round(res["torch_inverse"]["ms"] / res["xf_inverse"]["ms"], 2),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()),
                      "forward_max_difference_from_torch": float(f"{diff_f:.3e}"),
                      "inverse_max_difference_from_torch": float(f"{diff_i:.3e}")}), flush=True)


def generate(n_scenarios, per, repeats):
    conf = {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": 1000, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"]}, "generation": {}}
    md, ed, pd_ = 50, 1900, 50
    torch.manual_seed(0)
    model = BiologyAwareDiffusionModel(md, ed, pd_, 3, conf).cuda().eval()
    rs = np.random.default_rng(2)
    data = np.concatenate([rs.integers(0, 2, (1000, md)).astype(np.float32), cohort(1000, ed, 3), rs.normal(0, 1, (1000, pd_)).astype(np.float32)], axis=1)
    ft = FeatureTransform.fit(data, {"mutations": md, "expression": ed, "pathways": pd_}, {"expression": "quantile_normal", "pathways": "standard"})
    scenarios = [{"name": f"s{i}", "conditions": {"survival_time": 300 + 400 * i, "event_occurred": i % 2, "metastasis_at_diagnosis": i % 2}}
                 for i in range(n_scenarios)]
    gen = SyntheticPatientGenerator(model, conf, device="cuda")
    res = {}
    runs = {"generate_plain": [], "generate_transform": []}
    for rep in range(repeats + 1):
        for name, t in (("generate_plain", None), ("generate_transform", ft)):
            model.feature_transform = t
            dt = clock(lambda: res.__setitem__(name, gen.generate_scenarios(scenarios, per, seed=1)))
            if rep:                                             # the first round warms up
                runs[name].append(dt)
    model.feature_transform = None
    out = {name: stats(v) for name, v in runs.items()}
    for name, v in out.items():
        print(json.dumps({"case": name, "scenarios": n_scenarios, "per_scenario": per, "D": md + ed + pd_, "T": 1000, **v}), flush=True)
    expr = res["generate_transform"]["s0"]["expression"]
    print(json.dumps({"case": "generate_ratio", "transform_over_plain_time": round(out["generate_transform"]["ms"] / out["generate_plain"]["ms"], 4),
                      "added_ms": round(out["generate_transform"]["ms"] - out["generate_plain"]["ms"], 3),
                      "expression_min_with_transform": float(expr.min()),
                      "expression_min_plain": float(res["generate_plain"]["s0"]["expression"].min())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000x2000,100000x5142", help="rows x D of the kernel measurements")
    ap.add_argument("--levels", type=int, default=1000, help="Q: quantile levels per column")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--generate", default="3x1000", help="scenarios x patients of the end-to-end run; empty skips it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transform_bench measures on a GPU: none found")
    for size in (s for s in args.sizes.split(",") if s):
        rows, D = (int(v) for v in size.split("x"))
        kernel(rows, D, args.levels, args.repeats)
    if args.generate:
        n_sc, per = (int(v) for v in args.generate.split("x"))
        generate(n_sc, per, max(args.repeats // 2, 2))


if __name__ == "__main__":
    main()
