"""Price of training on incomplete patients: the training step (Trainer.train_step on a device-resident batch
source with mixup, as bench.py's training leg) at the BASELINE shape -- B = 4096, D = 2000 (50 / 1900 / 50, 3 conditions), hidden
[256, 512, 256], dropout 0.2 -- in ms per step from device events, one JSON line per variant plus one line of ratios.

  off      missing_values unset: the kernels of a build without the feature
  off_b    the same again, a second model and Trainer: the spread of `off` against itself
  on       missing_values: mask, no NaN in the data (masked q_sample + EpiLossT<true> in place of EpiMse)
  on30     missing_values: mask, 30 % of the patients without the expression block (whole-block NaN)

Every variant has its own model and Trainer; all are warmed up first (20 steps each), then the variants ALTERNATE inside this one
process: `--rounds` rounds, in each round every variant runs one window of `--steps` steps between two device events.  A line reports
the median window and the spread (min, max) in ms per step over rounds x steps >= 200 steps, so drift of the box lands on every
variant alike.

    python tools/mask_bench.py [--variants off,off_b,on,on30] [--rounds 8] [--steps 50]
"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from osteosarcoma_diffusionmodel_amd import BiologyAwareDiffusionModel  # noqa: E402
from osteosarcoma_diffusionmodel_amd.train import Trainer  # noqa: E402

B = 4096
ROWS = 65536
DIMS = (50, 1900, 50, 3)
VARIANTS = {"off": (None, 0.0), "off_b": (None, 0.0), "on": ("mask", 0.0), "on30": ("mask", 0.3)}


def config(save_dir, missing_values):
    conf = {"model": {"latent_dim": 128, "hidden_dims": [256, 512, 256], "gnn": {"dropout": 0.2},
                      "diffusion": {"num_steps": 1000, "beta_schedule": "cosine"},
                      "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"},
            "training": {"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.2},
                         "save_dir": save_dir, "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": B}}
    if missing_values is not None:
        conf["training"]["missing_values"] = missing_values
    return conf


class Runner:
    def __init__(self, variant, data, cond, surv, save_dir):
        mut, expr, pw, cd = DIMS
        missing_values, frac = VARIANTS[variant]
        conf = config(save_dir, missing_values)
        torch.manual_seed(0)
        self.model = BiologyAwareDiffusionModel(mut, expr, pw, cd, conf)
        self.tr = Trainer(self.model, [], [], conf, device="cuda")
        self.model.train()
        if frac > 0.0:
            data = data.clone()
            g = torch.Generator(device="cuda").manual_seed(7)
            rows = torch.rand(ROWS, device="cuda", generator=g) < frac
            data[rows, mut:mut + expr] = float("nan")
        self.observed = 1.0 - float(torch.isnan(data).double().mean())
        self.data, self.cond, self.surv = data, cond, surv
        self.order = torch.arange(ROWS, device="cuda", dtype=torch.int64)
        self.lams, self.perms, _ = self.tr.mixup.draw_epoch([B] * 64, "cuda")
        self.i = 0
        self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))

    def step(self):
        i = self.i
        self.i += 1
        o = (i * B) % (ROWS - B)
        idx = self.order[o:o + B]
        j = i % 64
        return self.tr.train_step(None, None, source=(self.data, self.cond, self.surv, idx, idx[self.perms[j]], self.lams[j]))

    def window(self, steps):
        """ms per step over `steps` steps between two device events."""
        torch.cuda.synchronize()
        self.ev[0].record()
        for _ in range(steps):
            self.step()
        self.ev[1].record()
        torch.cuda.synchronize()
        return self.ev[0].elapsed_time(self.ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="off,off_b,on,on30")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    if args.rounds * args.steps < 200:
        ap.error("rounds x steps must be at least 200 steps per figure")
    save_dir = tempfile.mkdtemp(prefix="osd_mask_bench_")
    D = sum(DIMS[:3])
    g = torch.Generator(device="cuda").manual_seed(42)
    data = torch.randn(ROWS, D, device="cuda", generator=g)
    data[:, :DIMS[0]] = (torch.rand(ROWS, DIMS[0], device="cuda", generator=g) < 0.5).float()
    cond = torch.randn(ROWS, DIMS[3], device="cuda", generator=g)
    surv = torch.rand(ROWS, device="cuda", generator=g)
    names = args.variants.split(",")
    runners = {v: Runner(v, data, cond, surv, save_dir) for v in names}
    for r in runners.values():
        for _ in range(20):
            r.step()
    torch.cuda.synchronize()
    wins = {v: [] for v in names}
    for _ in range(args.rounds):
        for v in names:
            wins[v].append(runners[v].window(args.steps))
    med = {}
    for v in names:
        w = sorted(wins[v])
        med[v] = w[len(w) // 2]
        print(json.dumps({"D": D, "batch": B, "variant": v, "missing_values": VARIANTS[v][0], "observed_fraction": round(runners[v].observed, 4),
                          "ms_per_step": round(med[v], 4), "ms_per_step_min": round(w[0], 4), "ms_per_step_max": round(w[-1], 4),
                          "spread_pct": round(100 * (w[-1] - w[0]) / med[v], 2), "steps": args.rounds * args.steps,
                          "loss": round(float(runners[v].step().item()), 5)}), flush=True)
    if "off" in med:
        print(json.dumps({"ratio_to_off": {v: round(med[v] / med["off"], 4) for v in names}}), flush=True)


if __name__ == "__main__":
    main()
