"""Price of the grouped clip + AdamW step (fine-tuning: per-group learning rate / weight decay, L2-SP anchor, frozen ranges).  One JSON line.

  optimizer step, us per step on flat buffers of n = 2 663 952 floats (the BASELINE shape: 50 / 1900 / 50, 3 conditions, hidden
  256 / 512 / 256), device events around windows of `--reps` back-to-back steps, every variant from this one library in this one process:
      plain        osd_nn_clip_adamw_step / _ema_step                                             7 (EMA: 9) streams of n floats + the norm's read
      one_group    the grouped step, one default group                                            the same streams
      per_tensor   one default group per parameter tensor (unmerged: the table's worst realistic size)
      anchor       one group with l2sp > 0                                                        + 1 stream (read anchor): 8/7 (EMA: 10/9)
      half_frozen  the tensors of the first half of the buffer frozen                             about half the streams; the norm still reads g
  each with and without the EMA.  `plain` appears twice (plain, plain_again) so that its own run-to-run spread is measured by the same
  script: the target for one_group is to lie within it.
  training step, ms per Trainer.train_step at B = 4096, D = 2000 on a device-resident batch source, with training.finetune (a frozen
  encoder and time projection, a scaled decoder, l2_sp) and without.

All variants are warmed up first and then ALTERNATE: `--rounds` rounds, each variant one window per round; a figure is the median
window with (min, max) next to it.

    python tools/finetune_bench.py [--reps 2000] [--rounds 7] [--window 0.5] [--no-train]
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
DIMS = (50, 1900, 50, 3)
HYPER = (1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0)      # lr, betas, eps, weight decay, max_norm: the Trainer's
DECAY = 0.999
FINETUNE = {"freeze": ["unet.encoder", "unet.time_proj"], "lr_scale": {"unet.decoder": 0.1}, "l2_sp": 0.01}


def tensor_numels():
    cfg = L.OsdConfig()
    cfg.mutation_dim, cfg.expression_dim, cfg.pathway_dim, cfg.condition_dim = DIMS
    cfg.time_dim, cfg.n_hidden = 128, len(HIDDEN)
    for i, v in enumerate(HIDDEN):
        cfg.hidden_dims[i] = v
    cfg.num_steps = 1000
    lib = L.lib()
    return [lib.osd_param_numel(C.byref(cfg), i) for i in range(lib.osd_num_params(C.byref(cfg)))]


def stats(wins, digits=3):
    w = sorted(wins)
    return {"median": round(w[len(w) // 2], digits), "min": round(w[0], digits), "max": round(w[-1], digits)}


def table(groups):
    tab = (L.OsdParamGroup * len(groups))()
    for k, g in enumerate(groups):
        tab[k] = L.OsdParamGroup(*g)
    return tab


class OptBench:
    def __init__(self, numels):
        g = torch.Generator(device="cuda").manual_seed(1)
        n = self.n = sum(numels)
        self.p = torch.randn(n, device="cuda", generator=g) * 0.05
        self.g = torch.randn(n, device="cuda", generator=g) * 0.01
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.e = self.p.clone()
        self.anchor = self.p.clone()
        self.ws = torch.zeros(L.OSD_GROUP_WS_DOUBLES, device="cuda", dtype=torch.float64)
        self.norm = torch.zeros(1, device="cuda")
        self.step = 0
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.dev = torch.cuda.current_device()
        ends = [0]
        for k in numels:
            ends.append(ends[-1] + k)
        half = min(ends[1:-1], key=lambda e: abs(e - n / 2))
        self.tables = {"one_group": table([(0, n, 1.0, 1.0, 0.0)]),
                       "per_tensor": table([(b, e, 1.0, 1.0, 0.0) for b, e in zip(ends, ends[1:])]),
                       "anchor": table([(0, n, 1.0, 1.0, 0.01)]),
                       "half_frozen": table([(0, half, 0.0, 1.0, 0.0), (half, n, 1.0, 1.0, 0.0)])}
        self.info = {"numel": n, "tensors": len(numels), "frozen_elements": half}

    def plain(self, ema):
        self.step += 1
        lr, b1, b2, eps, wd, mx = HYPER
        head = (self.stream, self.dev, L.ptr(self.ws), L.ptr(self.p), L.ptr(self.g), L.ptr(self.m), L.ptr(self.v))
        if ema:
            L.check(L.lib().osd_nn_clip_adamw_ema_step(*head, L.ptr(self.e), self.n, lr, b1, b2, eps, wd, mx, self.step, DECAY, L.ptr(self.norm)))
        else:
            L.check(L.lib().osd_nn_clip_adamw_step(*head, self.n, lr, b1, b2, eps, wd, mx, self.step, L.ptr(self.norm)))

    def grouped(self, name, ema):
        self.step += 1
        tab = self.tables[name]
        L.check(L.lib().osd_nn_group_adamw_step(self.stream, self.dev, L.ptr(self.ws), L.ptr(self.p), L.ptr(self.g), L.ptr(self.m), L.ptr(self.v),
                                                L.ptr(self.e if ema else None), L.ptr(self.anchor if name == "anchor" else None), self.n, tab,
                                                len(tab), *HYPER, self.step, DECAY if ema else 0.0, L.ptr(self.norm)))

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
        out = dict(self.info)
        for ema in (False, True):
            variants = {"plain": lambda: self.plain(ema), "plain_again": lambda: self.plain(ema)}
            for name in self.tables:
                variants[name] = lambda name=name: self.grouped(name, ema)
            for fn in variants.values():
                for _ in range(50):
                    fn()
            torch.cuda.synchronize()
            wins = {k: [] for k in variants}
            for _ in range(rounds):
                for k, fn in variants.items():
                    wins[k].append(self.window(fn, reps))
            res = {k: stats(w) for k, w in wins.items()}
            base = res["plain"]["median"]
            for k in list(variants)[1:]:
                res[f"{k}_over_plain"] = round(res[k]["median"] / base, 4)
            res["byte_ratio_anchor"] = round(10 / 9 if ema else 8 / 7, 4)
            out["ema" if ema else "no_ema"] = res
        return out


class TrainRunner:
    def __init__(self, data, cond, surv, save_dir, finetune):
        conf = {"model": {"latent_dim": 128, "hidden_dims": list(HIDDEN), "gnn": {"dropout": 0.2},
                          "diffusion": {"num_steps": 1000, "beta_schedule": "cosine"},
                          "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"},
                "training": {"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.2},
                             "save_dir": save_dir, "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": B}}
        if finetune:
            conf["training"]["finetune"] = dict(FINETUNE)
        torch.manual_seed(0)
        self.tr = Trainer(BiologyAwareDiffusionModel(*DIMS, conf), [], [], conf, device="cuda")
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
    D = sum(DIMS[:3])
    g = torch.Generator(device="cuda").manual_seed(42)
    data = torch.randn(ROWS, D, device="cuda", generator=g)
    data[:, :DIMS[0]] = (torch.rand(ROWS, DIMS[0], device="cuda", generator=g) < 0.5).float()
    cond = torch.randn(ROWS, DIMS[3], device="cuda", generator=g)
    surv = torch.rand(ROWS, device="cuda", generator=g)
    save_dir = tempfile.mkdtemp(prefix="osd_finetune_bench_")
    runners = {"plain": TrainRunner(data, cond, surv, save_dir, False), "finetune": TrainRunner(data, cond, surv, save_dir, True)}
    for r in runners.values():
        for _ in range(20):
            r.step()
    wins = {k: [] for k in runners}
    for _ in range(rounds):
        for k, r in runners.items():
            wins[k].append(r.window(seconds))
    out = {k: stats(w, 4) for k, w in wins.items()}
    out["groups"] = len(runners["finetune"].tr.optimizer._groups)
    out["finetune_over_plain"] = round(out["finetune"]["median"] / out["plain"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000, help="optimizer steps per window (at least 200)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per training-step window")
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    if args.reps < 200:
        ap.error("--reps must be at least 200")
    if not torch.cuda.is_available():
        raise SystemExit("finetune_bench needs the GPU: there is nothing to time without it")
    result = {"tool": "finetune_bench", "decay": DECAY, "reps_per_window": args.reps, "rounds": args.rounds,
              "optimizer_us_per_step": OptBench(tensor_numels()).run(args.reps, args.rounds)}
    torch.cuda.empty_cache()
    if not args.no_train:
        result["train_step_ms"] = {"batch": B, "D": 2000, **train_bench(args.rounds, args.window)}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
