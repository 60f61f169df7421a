"""Rate of the two subspace-iteration kernels (osd_val_pca_project, osd_val_pca_backproject; csrc/pca.hip) against their yardsticks on
the same tensors in the same process, a whole ``DevicePCA`` fit against the Gram route and against sklearn on the host, and
``statistical_tests`` / ``embedding_fidelity`` end to end (one JSON line per measurement).

  project      DeviceKernels.pca_project with the norms: one read of X, 2 n D l FLOPs in double
  backproject  DeviceKernels.pca_backproject on project's Z: one read of X, 2 n D l FLOPs
  pair         one after the other, an iteration of the fit: two reads, 4 n D l FLOPs
  copy         a device copy of X: one read and one write -- the floor of a pair is two reads
  torch_pair   the same definition in torch: u = (x.double() - c) * s, Z = u @ V, W = u.T @ Z; values compared with ours
  fit          DevicePCA(10).fit split into the kernel pairs, the moments, and the rest (host QR and eigh, transfers), against
               gram_eigh (osd_val_centered_gram + scipy.linalg.eigh(subset_by_index) on the host) and sklearn_host (the cohort
               downloaded, sklearn's PCA(10): what statistical_tests does by default)
  statistical_tests, embedding_fidelity     end to end on two planted cohorts

Each case warms up once, then times `--repeats` repeats bracketed by torch.cuda.synchronize(); the kernel cases alternate so that a
drift of the machine hits all alike.  A line reports the median, min and max, the spread (max - min) / median, the effective GB/s
of X (rows x D x 4 bytes per read) and the GFLOP/s.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python tools/pca_bench.py --sizes 125000x2000 --fit "" --e2e ""`.

    python tools/pca_bench.py [--sizes 125000x2000,100000x5142,3000x5142] [--l 18] [--repeats 7] [--fit 125000x2000,3000x5142]
                              [--e2e 125000x2000] [--gram-max-d 2500]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import pca as PC  # noqa: E402
from osteosarcoma_diffusionmodel_amd.validation import BiologicalValidator, DeviceKernels  # noqa: E402
from survival_bench import clock, parse_sizes, stats  # noqa: E402


def pair_flops(rows, D, l):
    """FLOPs of one project + backproject pair: two products of 2 n D l each."""
    return 4.0 * rows * D * l


def cohort(n, D, seed, shrink=1.0):
    """fp32 [n, D] on the device: a rank-12 factor model (score sd 6 .. 2.5, times ``shrink``) plus unit noise and an offset: the
    ten directions the reference asks for lie inside the planted spectrum."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    basis = torch.linalg.qr(torch.randn(D, 12, device="cuda", generator=torch.Generator(device="cuda").manual_seed(99)))[0]
    sd = torch.linspace(6.0, 2.5, 12, device="cuda") * shrink
    x = (torch.randn(n, 12, device="cuda", generator=g) * sd) @ basis.T + torch.randn(n, D, device="cuda", generator=g) + 3.0
    return x.contiguous()


def kernel(rows, D, l, repeats):
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x = cohort(rows, D, 1)
    c = x.double().mean(0)
    s = 1.0 / x.double().std(0)
    V = torch.linalg.qr(torch.randn(D, l, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)))[0]
    z0, _ = k.pca_project(x, c, s, V, norm2=True)
    sink = torch.empty_like(x)

    def torch_pair():
        u = (x.double() - c) * s
        z = u @ V
        return z, u.T @ z

    def pair():
        z, _ = k.pca_project(x, c, s, V, norm2=True)
        return z, k.pca_backproject(x, c, s, z)

    calls = {"project": lambda: k.pca_project(x, c, s, V, norm2=True), "backproject": lambda: k.pca_backproject(x, c, s, z0),
             "pair": pair, "copy": lambda: sink.copy_(x), "torch_pair": torch_pair}
    for fn in calls.values():
        fn()
    (z, w), (zt, wt) = pair(), torch_pair()
    rel = [float((a - b).abs().max() / b.abs().max()) for a, b in ((z, zt), (w, wt))]
    del zt, wt
    runs = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            runs[name].append(clock(fn))
    x_bytes = 4.0 * rows * D
    reads = {"project": 1, "backproject": 1, "pair": 2, "copy": 2, "torch_pair": 2}
    flops = {"project": 0.5, "backproject": 0.5, "pair": 1.0, "torch_pair": 1.0}
    res = {}
    for name, v in runs.items():
        res[name] = stats(v, reads[name] * x_bytes)
        if name in flops:
            res[name]["gflop_per_s"] = round(flops[name] * pair_flops(rows, D, l) / (res[name]["ms"] * 1e-3) / 1e9, 1)
        print(json.dumps({"case": name, "rows": rows, "D": D, "l": l, "x_mb": round(x_bytes / 1e6, 1), "x_passes": reads[name],
                          **res[name]}), flush=True)
    ratio = lambda a, b: round(res[a]["ms"] / res[b]["ms"], 4)
    print(json.dumps({"case": "ratio", "rows": rows, "D": D, "l": l, "pair_over_copy_time": ratio("pair", "copy"),
                      "project_over_copy_time": ratio("project", "copy"), "backproject_over_copy_time": ratio("backproject", "copy"),
                      "pair_over_torch_pair_time": ratio("pair", "torch_pair"),
                      "larger_spread_pct": max(v["spread_pct"] for v in res.values()),
                      "Z_W_max_rel_difference_to_torch": [float(f"{v:.3e}") for v in rel]}), flush=True)


class Timed:
    """DeviceKernels that adds up the wall time of its calls (each is synchronous)."""

    def __init__(self, k):
        self.k, self.t = k, {"col_moments64": 0.0, "pca_project": 0.0, "pca_backproject": 0.0}

    def __getattr__(self, name):
        fn = getattr(self.k, name)
        if name not in self.t:
            return fn

        def timed(*a, **kw):
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            self.t[name] += time.perf_counter() - t0
            return out
        return timed


def fit(rows, D, repeats, gram_max_d):
    from scipy.linalg import eigh
    from sklearn.decomposition import PCA
    k = DeviceKernels(torch.device("cuda", torch.cuda.current_device()))
    x = cohort(rows, D, 1)
    PC.DevicePCA(10).fit(x, kernels=k)
    runs, parts, last = [], [], None
    for _ in range(repeats):
        tk = Timed(k)
        box = {}
        runs.append(clock(lambda: box.setdefault("fit", PC.DevicePCA(10).fit(x, kernels=tk))))
        parts.append(dict(tk.t))
        last = box["fit"]
    mid = int(np.argsort(runs)[len(runs) // 2])
    pairs_ms = 1e3 * (parts[mid]["pca_project"] + parts[mid]["pca_backproject"])
    line = {"case": "fit", "rows": rows, "D": D, "k": 10, "l": int(last.initial_basis(D).shape[1]), "iterations": int(last.n_iter_),
            "converged": bool(last.converged_), **stats(runs), "pairs_ms": round(pairs_ms, 3),
            "moments_ms": round(1e3 * parts[mid]["col_moments64"], 3),
            "host_qr_eigh_transfers_ms": round(1e3 * runs[mid] - pairs_ms - 1e3 * parts[mid]["col_moments64"], 3)}
    print(json.dumps(line), flush=True)
    if D <= gram_max_d:
        def gram_route():
            mean = x.double().mean(0)
            g = k.centered_gram(x, mean.float().cpu().numpy()).cpu().numpy()
            return eigh(g, subset_by_index=[D - 10, D - 1])[0][::-1] / (rows - 1)
        lam = gram_route()
        g_runs = [clock(gram_route) for _ in range(max(repeats // 2, 2))]
        print(json.dumps({"case": "gram_eigh", "rows": rows, "D": D, **stats(g_runs),
                          "eigenvalue_max_rel_difference": float(f"{np.abs(lam / last.explained_variance_ - 1).max():.3e}")}), flush=True)
    else:
        print(json.dumps({"case": "gram_eigh", "rows": rows, "D": D, "ms": "not measured"}), flush=True)

    def sklearn_host():
        return PCA(n_components=10).fit(x.cpu().numpy())
    sk = sklearn_host()
    s_runs = [clock(sklearn_host) for _ in range(2)]
    print(json.dumps({"case": "sklearn_host", "rows": rows, "D": D, **stats(s_runs),
                      "eigenvalue_max_rel_difference": float(f"{np.abs(sk.explained_variance_ / last.explained_variance_ - 1).max():.3e}")}),
          flush=True)


def end_to_end(rows, D, repeats):
    val = BiologicalValidator({"evaluation": {}})
    real, synth = cohort(rows, D, 2), cohort(rows, D, 3, shrink=0.8)
    for mode in ("host", "device"):
        box = {}

        def tests():
            np.random.seed(0)
            box["r"] = val.statistical_tests(real, synth, pca=mode)
        tests()
        runs = [clock(tests) for _ in range(repeats)]
        print(json.dumps({"case": "statistical_tests", "pca": mode, "rows_per_cohort": rows, "D": D, **stats(runs),
                          "wasserstein_distance_mean": round(box["r"]["wasserstein_distance_mean"], 6)}), flush=True)
    box = {}

    def embedding():
        box["r"] = val.embedding_fidelity(real, synth)
    embedding()
    runs = [clock(embedding) for _ in range(repeats)]
    shown = {key: (round(v, 4) if isinstance(v, float) else v) for key, v in box["r"].items()
             if key in ("pca_iterations_real", "pca_iterations_synth", "pca_converged", "pca_variance_ratio_mean", "pca_offmanifold_share",
                        "pca_subspace_cos_min", "pca_wasserstein_distance_mean")}
    print(json.dumps({"case": "embedding_fidelity", "rows_per_cohort": rows, "D": D, **stats(runs), **shown}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="125000x2000,100000x5142,3000x5142", help="rows x D of the kernel measurements")
    ap.add_argument("--l", type=int, default=18, help="directions of the kernel measurements")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fit", default="125000x2000,3000x5142", help="rows x D of the fit measurements; empty skips them")
    ap.add_argument("--e2e", default="125000x2000", help="rows x D of the end-to-end runs; empty skips them")
    ap.add_argument("--gram-max-d", type=int, default=2500, help="widest cohort the Gram + eigh route is timed on")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench measures on a GPU: none found")
    for rows, D in parse_sizes(args.sizes):
        kernel(rows, D, args.l, args.repeats)
    for rows, D in parse_sizes(args.fit):
        fit(rows, D, max(args.repeats // 2, 3), args.gram_max_d)
    for rows, D in parse_sizes(args.e2e):
        end_to_end(rows, D, max(args.repeats // 3, 2))


if __name__ == "__main__":
    main()
