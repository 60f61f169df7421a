"""Price of differentially private training (training.dp).  One JSON line.

  training step, ms per Trainer.train_step at B = 4096, D = 2000, hidden 256 / 512 / 256 on a device-resident batch source (mixup off in
      both: DP refuses it), without and with training.dp;
  the two DP launches on their own, us and TB/s (device events around `--reps` back-to-back launches on the step's own buffers): the
      row-norm launch (bytes = every row it reads) and the clip-factor launch with every row clipped (bytes = read + write of every
      scaled row; a row with c_r = 1 is skipped altogether, so a step moves at most this);
  optimizer step, us on the flat parameter buffer: clip + AdamW (k_sumsq + k_adamw) against the DP step (k_adamw_dp).

Variants are warmed up first and then ALTERNATE inside this one process, `--rounds` rounds; a figure is the median window with (min,
max) next to it.  --no-dp times the non-DP training step alone: the figure to set beside the same run of another commit's checkout
(alternate the two processes in one session), since one process cannot host two builds of the package.

    python tools/dp_bench.py [--rounds 7] [--window 0.5] [--reps 500] [--no-dp]
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
D = sum(DIMS[:3])
COPY_TBS = 6.29          # the float4 copy rate the microarchitecture guide measured on this part, TB/s


def stats(wins, digits=4):
    w = sorted(wins)
    return {"median": round(w[len(w) // 2], digits), "min": round(w[0], digits), "max": round(w[-1], digits)}


def dp_bytes():
    """(bytes the row-norm launch reads, bytes the clip launch moves when every row is clipped) per step at B rows."""
    H0, widths = HIDDEN[0], list(HIDDEN[1:]) + [HIDDEN[-1]] + list(HIDDEN[-2::-1])
    n_enc = len(HIDDEN) - 1
    read = widths[-1] + D                                   # output_proj: x, delta
    scale = D
    outs = []
    for b, c in enumerate(widths):
        k1 = H0 if b == 0 else widths[b - 1]
        k2 = outs[n_enc - 1 - (b - n_enc - 1)] if b > n_enc else 0
        read += (c + c) + (k1 + k2 + c)                    # second Linear: mid, g_z2; first: main + skip inputs, g_z1
        read += 2 * (2 * c + 16)                           # two GroupNorm layers: gy, z, stats
        scale += 4 * c
        outs.append(c)
    read += D + 64 + 128 + H0 + (64 + 64) + (DIMS[3] + 64)  # h0's three Linears on g_h0; the two embedding Linears
    scale += H0 + 64 + 64
    return 4 * B * read, 2 * 4 * B * scale


class TrainRunner:
    def __init__(self, data, cond, surv, save_dir, dp):
        conf = {"model": {"latent_dim": 128, "hidden_dims": list(HIDDEN), "gnn": {"dropout": 0.2},
                          "diffusion": {"num_steps": 1000, "beta_schedule": "cosine"},
                          "condition_on": ["survival_time", "event_occurred", "metastasis_at_diagnosis"], "architecture": "diffusion"},
                "training": {"learning_rate": 1e-4, "weight_decay": 1e-5, "patience": 100, "min_delta": 1e-4, "augmentation": {"mixup_alpha": 0.0},
                             "save_dir": save_dir, "num_epochs": 1, "save_frequency": 10, "val_split": 0.2, "random_seed": 42, "batch_size": B}}
        if dp:
            conf["training"]["dp"] = dp
        torch.manual_seed(0)
        self.tr = Trainer(BiologyAwareDiffusionModel(*DIMS, conf), [], [], conf, device="cuda")
        self.tr.model.train()
        self.data, self.cond, self.surv = data, cond, surv
        self.order = torch.arange(ROWS, device="cuda", dtype=torch.int64)
        self.i = 0

    def step(self):
        o = (self.i * B) % (ROWS - B)
        self.i += 1
        return self.tr.train_step(None, None, source=(self.data, self.cond, self.surv, self.order[o:o + B], None, 1.0))

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


def event_window(fn, reps):
    """us per call over `reps` back-to-back calls, by device events."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps


def launch_bench(runner, reps, rounds):
    """The step's two DP launches alone, replayed (osd_dp_replay) on the buffers the runner's last step left.  The clip launch runs with
    every factor just below 1, so that it reads and writes every row and the values stay put over the repeats."""
    lib = L.lib()
    h = runner.tr._engine.handle
    L.check(lib.osd_dp_replay(h, 2, 1.0 - 2.0 ** -24))
    out = {}
    read, moved = dp_bytes()
    for name, which, nbytes in (("clip_rows_all_clipped", 1, moved), ("row_norms", 0, read)):
        fn = lambda: L.check(lib.osd_dp_replay(h, which, 0.0))
        for _ in range(20):
            fn()
        wins = [event_window(fn, reps) for _ in range(rounds)]
        st = stats(wins, 2)
        st["bytes"] = nbytes
        st["TB_per_s"] = round(nbytes / (st["median"] * 1e-6) / 1e12, 3)
        st["share_of_copy_rate"] = round(st["TB_per_s"] / COPY_TBS, 3)
        out[name] = st
    return out


def optimizer_bench(n, reps, rounds):
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(n, device="cuda", generator=g) * 0.05
    gr = torch.randn(n, device="cuda", generator=g) * 0.01
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws, norm = torch.zeros(256, device="cuda", dtype=torch.float64), torch.zeros(1, device="cuda")
    stream, dev = C.c_void_p(torch.cuda.current_stream().cuda_stream), torch.cuda.current_device()
    lib = L.lib()
    step = [0]

    def plain():
        step[0] += 1
        L.check(lib.osd_nn_clip_adamw_step(stream, dev, L.ptr(ws), L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), n, 1e-4, 0.9, 0.999, 1e-8, 1e-5, 1.0,
                                           step[0], L.ptr(norm)))

    def dp():
        step[0] += 1
        L.check(lib.osd_nn_dp_adamw_step(stream, dev, L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), n, 1e-4, 0.9, 0.999, 1e-8, 1e-5, 1e-4, 7, step[0]))

    variants = {"clip_adamw": plain, "dp_adamw": dp}
    for fn in variants.values():
        for _ in range(50):
            fn()
    wins = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            wins[k].append(event_window(fn, reps))
    out = {k: stats(w, 2) for k, w in wins.items()}
    out["numel"] = n
    out["dp_over_clip"] = round(out["dp_adamw"]["median"] / out["clip_adamw"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per training-step window")
    ap.add_argument("--reps", type=int, default=500, help="launches per window of the kernel and optimizer figures")
    ap.add_argument("--no-dp", action="store_true", help="the non-DP training step only (any build of the library, e.g. the parent's via OSDIFF_LIB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dp_bench needs the GPU: there is nothing to time without it")
    g = torch.Generator(device="cuda").manual_seed(42)
    data = torch.randn(ROWS, D, device="cuda", generator=g)
    data[:, :DIMS[0]] = (torch.rand(ROWS, DIMS[0], device="cuda", generator=g) < 0.5).float()
    cond = torch.randn(ROWS, DIMS[3], device="cuda", generator=g)
    surv = torch.rand(ROWS, device="cuda", generator=g)
    save_dir = tempfile.mkdtemp(prefix="osd_dp_bench_")
    runners = {"plain": TrainRunner(data, cond, surv, save_dir, None)}
    if not args.no_dp:
        # C = the median row norm of a first batch (the usual pick: about half of the rows clipped), sigma = 1.1
        probe = TrainRunner(data, cond, surv, save_dir, {"max_grad_norm": 1e30, "noise_multiplier": 0.0})
        probe.step()
        clip = float(probe.tr.last_row_norms().median().item())
        del probe
        runners["dp"] = TrainRunner(data, cond, surv, save_dir, {"max_grad_norm": clip, "noise_multiplier": 1.1, "seed": 7})
    for r in runners.values():
        for _ in range(20):
            r.step()
    wins = {k: [] for k in runners}
    for _ in range(args.rounds):
        for k, r in runners.items():
            wins[k].append(r.window(args.window))
    result = {"tool": "dp_bench", "batch": B, "D": D, "hidden": list(HIDDEN), "rounds": args.rounds,
              "train_step_ms": {k: stats(w) for k, w in wins.items()}}
    if not args.no_dp:
        ts = result["train_step_ms"]
        ts["max_grad_norm"] = round(clip, 5)
        ts["dp_over_plain"] = round(ts["dp"]["median"] / ts["plain"]["median"], 4)
        result["dp_launches_us"] = launch_bench(runners["dp"], args.reps, args.rounds)
        result["optimizer_us_per_step"] = optimizer_bench(runners["dp"].tr.flat.flat.numel(), args.reps, args.rounds)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
