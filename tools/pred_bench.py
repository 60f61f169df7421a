"""Price of the prediction types (config['model']['diffusion']['prediction_type']): one JSON line per measurement.

  --mode train     Trainer.train_step on a device-resident batch source (bench.py's training leg) at B = 4096 for epsilon (the default:
                   the kernels of the commit before the feature), v_prediction and sample, at D2000 (50 / 1900 / 50) and at the real dims
                   (62 / 5054 / 26).  Every variant has its own model and Trainer over the same data; all are warmed up, then they
                   ALTERNATE inside this process in windows of at least --window seconds (tools/loss_bench.py's procedure); in every mode
                   the order of the variants rotates from round to round.
  --mode qsample   k_q_sample<kind> alone (osd_q_sample_target on 4096 rows, device events over 200 launches, the kinds alternating) in us.
                   k_q_sample_src<kind> runs only inside the training call: take it from `rocprofv3 --kernel-trace --stats` of --mode train.
  --mode sample    ms per reverse step of a v_prediction model against an epsilon model on each engine (same kernels, other tables).
  --mode step      the default training step of THIS tree, alone: ms per step of one window (what --mode ab runs in each child).
  --mode ab        the default training step of this tree against another checkout with its library built (--parent PATH, e.g. the parent
                   commit): fresh child processes of `--mode step`, the two trees alternating, --runs runs each (7), median and spread.

    python tools/pred_bench.py --mode train [--dims D2000,real] [--rounds 5] [--window 1.0]
    python tools/pred_bench.py --mode ab --parent ../parent_checkout [--dims D2000,real] [--runs 7]
"""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
B = 4096
ROWS = 65536
DIMS = {"D2000": (50, 1900, 50, 3), "real": (62, 5054, 26, 4)}
TYPES = ("epsilon", "v_prediction", "sample")
ENGINES = {"layers_graph": ("graph", True, None, None), "layers_eager": ("graph", False, None, None), "workspace": ("chain", True, "workspace", None),
           "panel": ("chain", True, "panel", None), "squad32": ("chain", True, "squad", 32), "squad16": ("chain", True, "squad", 16)}


def config(save_dir, T=1000, prediction=None):
    diffusion = {"num_steps": T, "beta_schedule": "cosine"}
    if prediction is not None and prediction != "epsilon":          # epsilon: no key, the config of the commit before the feature
        diffusion["prediction_type"] = prediction
    return {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2}, "diffusion": diffusion,
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"},
            "training": {"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.2},
                         "save_dir": save_dir, "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": B}}


def dataset(dims):
    D = sum(dims[:3])
    g = torch.Generator(device="cuda").manual_seed(42)
    data = torch.randn(ROWS, D, device="cuda", generator=g)
    data[:, :dims[0]] = (torch.rand(ROWS, dims[0], device="cuda", generator=g) < 0.5).float()
    return data, torch.randn(ROWS, dims[3], device="cuda", generator=g), torch.rand(ROWS, device="cuda", generator=g)


class Runner:
    def __init__(self, dims, prediction, data, cond, surv, save_dir):
        from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
        from osteosarcoma_diffusionmodel_amd.train import Trainer
        mut, expr, pw, cd = dims
        conf = config(save_dir, prediction=prediction)
        torch.manual_seed(0)
        self.model = BiologyAwareDiffusionModel(mut, expr, pw, cd, conf)
        self.tr = Trainer(self.model, [], [], conf, device="cuda")
        self.model.train()
        self.data, self.cond, self.surv = data, cond, surv
        self.order = torch.arange(ROWS, device="cuda", dtype=torch.int64)
        self.lams, self.perms, _ = self.tr.mixup.draw_epoch([B] * 64, "cuda")
        self.i = 0

    def step(self):
        i = self.i
        self.i += 1
        o = (i * B) % (ROWS - B)
        idx = self.order[o:o + B]
        j = i % 64
        return self.tr.train_step(None, None, source=(self.data, self.cond, self.surv, idx, idx[self.perms[j]], self.lams[j]))

    def window(self, seconds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        while True:
            for _ in range(50):
                self.step()
            n += 50
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return 1e3 * dt / n


def rotated(names, i):
    """The round's order: every variant takes every position in turn, so that what runs before it is not always the same variant."""
    k = i % len(names)
    return names[k:] + names[:k]


def stats(values):
    w = sorted(values)
    med = w[len(w) // 2]
    return {"median": round(med, 4), "min": round(w[0], 4), "max": round(w[-1], 4), "spread_pct": round(100 * (w[-1] - w[0]) / med, 2), "n": len(w)}


def mode_train(args):
    save_dir = tempfile.mkdtemp(prefix="osd_pred_bench_")
    for dname in args.dims.split(","):
        dims = DIMS[dname]
        data, cond, surv = dataset(dims)
        runners = {p: Runner(dims, p, data, cond, surv, save_dir) for p in TYPES}
        for r in runners.values():
            for _ in range(20):
                r.step()
        torch.cuda.synchronize()
        wins = {p: [] for p in TYPES}
        for i in range(args.rounds):
            for p in rotated(TYPES, i):
                wins[p].append(runners[p].window(args.window))
        res = {p: stats(wins[p]) for p in TYPES}
        for p in TYPES:
            print(json.dumps({"mode": "train", "dims": dname, "batch": B, "prediction_type": p, "ms_per_step": res[p],
                              "loss": round(float(runners[p].step().item()), 5)}), flush=True)
        print(json.dumps({"mode": "train", "dims": dname, "ratio_to_epsilon": {p: round(res[p]["median"] / res["epsilon"]["median"], 4) for p in TYPES}}),
              flush=True)
        del runners
        torch.cuda.empty_cache()


def mode_step(args):
    save_dir = tempfile.mkdtemp(prefix="osd_pred_bench_")
    for dname in args.dims.split(","):
        dims = DIMS[dname]
        r = Runner(dims, None, *dataset(dims), save_dir)
        for _ in range(40):
            r.step()
        print(json.dumps({"mode": "step", "dims": dname, "ms_per_step": round(r.window(args.window), 4)}), flush=True)
        del r
        torch.cuda.empty_cache()


def mode_ab(args):
    trees = {"this": ROOT, "parent": Path(args.parent).resolve()}
    got = {k: {d: [] for d in args.dims.split(",")} for k in trees}
    for _ in range(args.runs):
        for k, tree in trees.items():
            out = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--mode", "step", "--dims", args.dims, "--window", str(args.window),
                                  "--tree", str(tree)], capture_output=True, text=True, check=True).stdout
            for ln in out.splitlines():
                rec = json.loads(ln)
                got[k][rec["dims"]].append(rec["ms_per_step"])
                print(f"{k}: {ln}", file=sys.stderr, flush=True)
    for d in args.dims.split(","):
        a, b = stats(got["this"][d]), stats(got["parent"][d])
        print(json.dumps({"mode": "ab", "dims": d, "batch": B, "this_ms_per_step": a, "parent_ms_per_step": b,
                          "this_over_parent": round(a["median"] / b["median"], 4)}), flush=True)


def mode_qsample(args):
    from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, _lib as L
    for dname in args.dims.split(","):
        mut, expr, pw, cd = DIMS[dname]
        D = mut + expr + pw
        models = {}
        for p in TYPES:
            models[p] = BiologyAwareDiffusionModel(mut, expr, pw, cd, config("", prediction=p)).cuda().eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        x0 = torch.randn(B, D, device="cuda", generator=g)
        t = torch.randint(0, 1000, (B,), device="cuda", generator=g).to(torch.int32)
        x_t, target = torch.empty_like(x0), torch.empty_like(x0)
        times = {p: [] for p in TYPES}

        def launches(p, n):
            h = models[p]._engine().handle
            for _ in range(n):
                L.check(L.lib().osd_q_sample_target(h, L.ptr(x0), L.ptr(t), None, B, 7, 0, L.ptr(x_t), L.ptr(target)))

        for p in TYPES:
            launches(p, 20)
        for i in range(args.rounds):
            for p in rotated(TYPES, i):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launches(p, 200)
                e1.record()
                e1.synchronize()
                times[p].append(1e3 * e0.elapsed_time(e1) / 200)
        bytes_moved = 3 * B * D * 4          # x0 in, x_t and the target out (Philox noise)
        for p in TYPES:
            s = stats(times[p])
            print(json.dumps({"mode": "qsample", "dims": dname, "rows": B, "prediction_type": p, "us_per_launch": s,
                              "TB_per_s": round(bytes_moved / (s["median"] * 1e-6) / 1e12, 3)}), flush=True)


def mode_sample(args):
    from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel
    T, S = 1000, 50
    torch.manual_seed(0)
    models = {p: BiologyAwareDiffusionModel(50, 1900, 50, 3, config("", T=T, prediction=p)).cuda().eval() for p in ("epsilon", "v_prediction")}
    models["v_prediction"].load_state_dict(models["epsilon"].state_dict())
    for engine, (sampler, graph, variant, panel) in ENGINES.items():
        n = {"workspace": 65536, "panel": 16384, "squad32": 2048, "squad16": 512}.get(engine, 4096)
        cond = torch.randn(n, 3, device="cuda")
        times = {p: [] for p in models}
        for m in models.values():
            m.sampler, m.use_graph, m.chain_variant, m.squad_panel, m.input_splitk = sampler, graph, variant, panel, 0
            m.sample(cond, n, seed=1, num_inference_steps=S)
        for i in range(args.rounds):
            for p in rotated(tuple(models), i):
                m = models[p]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.sample(cond, n, seed=1, num_inference_steps=S)
                torch.cuda.synchronize()
                times[p].append(1e3 * (time.perf_counter() - t0) / S)
        res = {p: stats(times[p]) for p in models}
        print(json.dumps({"mode": "sample", "engine": engine, "rows": n, "steps": S, "ms_per_step": res,
                          "v_over_epsilon": round(res["v_prediction"]["median"] / res["epsilon"]["median"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["train", "qsample", "sample", "step", "ab"], default="train")
    ap.add_argument("--dims", default="D2000,real")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--parent", default="")
    ap.add_argument("--tree", default=str(ROOT), help="checkout whose package and library --mode step imports (used by --mode ab)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.tree).resolve()))
    if args.mode == "ab" and not args.parent:
        ap.error("--mode ab needs --parent PATH")
    {"train": mode_train, "qsample": mode_qsample, "sample": mode_sample, "step": mode_step, "ab": mode_ab}[args.mode](args)


if __name__ == "__main__":
    main()
