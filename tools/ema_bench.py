"""Price of the weight average (EMA) kept inside the fused clip + AdamW kernel.  One JSON line.

  optimizer step, us per step on flat buffers of n floats (device events around windows of `--reps` back-to-back steps), for
      a  no average                       k_sumsq + k_adamw<false>                       (1 + 7) streams of n floats
      b  the average in the same pass     k_sumsq + k_adamw<true>                        (1 + 9)
      c  a, then shadow.lerp_(flat, w)    the average as a second launch                 (1 + 7 + 3)
    at n = 2 663 952 (the BASELINE shape: 50 / 1900 / 50, 3 conditions) and at the flat-parameter count of the real dims
    (62 / 5054 / 26, 4 conditions), hidden 256 / 512 / 256 both.  With --baseline-lib PATH a fourth variant `base` runs a through
    another build of libosdiff.so (the commit before the feature) on the same buffers.
  training step, ms per Trainer.train_step at B = 4096, D = 2000 on a device-resident batch source, with and without the average.

All variants are warmed up first and then ALTERNATE inside this one process: `--rounds` rounds, each variant one window per round.
A figure is the median window with (min, max) next to it, so the spread of a variant's own repeats is there to judge a difference by.

    python tools/ema_bench.py [--reps 2000] [--rounds 7] [--window 0.5] [--baseline-lib path/to/libosdiff.so] [--no-train]
"""
import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel, _lib as L  # noqa: E402
from osteosarcoma_diffusionmodel_amd.train import Trainer  # noqa: E402

B = 4096
ROWS = 65536
HIDDEN = (256, 512, 256)
DIMS = {"D2000": (50, 1900, 50, 3), "real": (62, 5054, 26, 4)}
HYPER = (1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0)      # lr, betas, eps, weight decay, max_norm: the Trainer's
DECAY = 0.999


def flat_numel(dims):
    cfg = L.OsdConfig()
    cfg.mutation_dim, cfg.expression_dim, cfg.pathway_dim, cfg.condition_dim = dims
    cfg.time_dim, cfg.n_hidden = 128, len(HIDDEN)
    for i, v in enumerate(HIDDEN):
        cfg.hidden_dims[i] = v
    cfg.num_steps = 1000
    lib = L.lib()
    return sum(lib.osd_param_numel(C.byref(cfg), i) for i in range(lib.osd_num_params(C.byref(cfg))))


def stats(wins, digits=3):
    w = sorted(wins)
    return {"median": round(w[len(w) // 2], digits), "min": round(w[0], digits), "max": round(w[-1], digits)}


class OptBench:
    def __init__(self, n, baseline):
        g = torch.Generator(device="cuda").manual_seed(1)
        self.n = n
        self.p = torch.randn(n, device="cuda", generator=g) * 0.05
        self.g = torch.randn(n, device="cuda", generator=g) * 0.01
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.e_fused, self.e_sep = self.p.clone(), self.p.clone()
        self.ws = torch.zeros(256, device="cuda", dtype=torch.float64)
        self.norm = torch.zeros(1, device="cuda")
        self.step = 0
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.dev = torch.cuda.current_device()
        self.plain = L.lib().osd_nn_clip_adamw_step
        self.base = None
        if baseline:
            self.base = C.CDLL(str(baseline)).osd_nn_clip_adamw_step
            self.base.restype, self.base.argtypes = L._SIGNATURES["osd_nn_clip_adamw_step"]

    def _plain(self, fn):
        self.step += 1
        L.check(fn(self.stream, self.dev, L.ptr(self.ws), L.ptr(self.p), L.ptr(self.g), L.ptr(self.m), L.ptr(self.v), self.n, *HYPER,
                   self.step, L.ptr(self.norm)))

    def a(self):
        self._plain(self.plain)

    def base_(self):
        self._plain(self.base)

    def b(self):
        self.step += 1
        lr, b1, b2, eps, wd, mx = HYPER
        L.check(L.lib().osd_nn_clip_adamw_ema_step(self.stream, self.dev, L.ptr(self.ws), L.ptr(self.p), L.ptr(self.g), L.ptr(self.m),
                                                   L.ptr(self.v), L.ptr(self.e_fused), self.n, lr, b1, b2, eps, wd, mx, self.step, DECAY,
                                                   L.ptr(self.norm)))

    def c(self):
        self._plain(self.plain)
        self.e_sep.lerp_(self.p, 1.0 - DECAY)

    def window(self, fn, reps):
        """us per step over `reps` back-to-back steps, by device events."""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return 1e3 * t0.elapsed_time(t1) / reps

    def run(self, reps, rounds):
        variants = {"a": self.a, "b": self.b, "c": self.c}
        if self.base is not None:
            variants["base"] = self.base_
        for fn in variants.values():
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        wins = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                wins[k].append(self.window(fn, reps))
        out = {k: stats(w) for k, w in wins.items()}
        out["b_over_a"] = round(out["b"]["median"] / out["a"]["median"], 4)
        out["c_over_a"] = round(out["c"]["median"] / out["a"]["median"], 4)
        if "base" in out:
            out["a_over_base"] = round(out["a"]["median"] / out["base"]["median"], 4)
        return out


class TrainRunner:
    def __init__(self, data, cond, surv, save_dir, ema):
        conf = {"model": {"latent_dim": 128, "hidden_dims": list(HIDDEN), "gnn": {"dropout": 0.2},
                          "diffusion": {"num_steps": 1000, "beta_schedule": "cosine"},
                          "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"},
                "training": {"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.2},
                             "save_dir": save_dir, "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": B}}
        if ema:
            conf["training"]["ema_decay"] = DECAY
        torch.manual_seed(0)
        self.tr = Trainer(BiologyAwareDiffusionModel(*DIMS["D2000"], conf), [], [], conf, device="cuda")
        self.tr.model.train()
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
        """ms per step over whole steps lasting at least `seconds`."""
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


def train_bench(rounds, seconds):
    dims = DIMS["D2000"]
    D = sum(dims[:3])
    g = torch.Generator(device="cuda").manual_seed(42)
    data = torch.randn(ROWS, D, device="cuda", generator=g)
    data[:, :dims[0]] = (torch.rand(ROWS, dims[0], device="cuda", generator=g) < 0.5).float()
    cond = torch.randn(ROWS, dims[3], device="cuda", generator=g)
    surv = torch.rand(ROWS, device="cuda", generator=g)
    save_dir = tempfile.mkdtemp(prefix="osd_ema_bench_")
    runners = {"no_ema": TrainRunner(data, cond, surv, save_dir, False), "ema": TrainRunner(data, cond, surv, save_dir, True)}
    for r in runners.values():
        for _ in range(20):
            r.step()
    wins = {k: [] for k in runners}
    for _ in range(rounds):
        for k, r in runners.items():
            wins[k].append(r.window(seconds))
    out = {k: stats(w, 4) for k, w in wins.items()}
    out["ema_over_no_ema"] = round(out["ema"]["median"] / out["no_ema"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000, help="optimizer steps per window (at least 200)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per training-step window")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if args.reps < 200:
        ap.error("--reps must be at least 200")
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs the GPU: there is nothing to time without it")
    result = {"tool": "ema_bench", "decay": DECAY, "reps_per_window": args.reps, "rounds": args.rounds, "optimizer_us_per_step": {}}
    for name, dims in DIMS.items():
        n = flat_numel(dims)
        result["optimizer_us_per_step"][name] = {"numel": n, **OptBench(n, args.baseline_lib).run(args.reps, args.rounds)}
        torch.cuda.empty_cache()
    if not args.no_train:
        result["train_step_ms"] = {"batch": B, "D": 2000, **train_bench(args.rounds, args.window)}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
