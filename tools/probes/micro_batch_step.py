"""What gradient accumulation costs in the step: ms per `Trainer.train_step` and peak allocated bytes at the bench's synthetic B = 32 on one
GPU, unsplit (micro_batch = None: the path without accumulation) against 2 x 16 and 4 x 8, ONE model and ONE Trainer in one process.
Phase 1: the unsplit step alone (warm-up, then its peak: no accumulator has been allocated yet).  Phase 2: the variants alternated
round by round, a host clock around each step ending in a device synchronise; median and interquartile range per variant, and the
peak of each variant's steps (the split variants' includes the f32 accumulators, 4 B per parameter, which stay allocated).
usage: python tools/probes/micro_batch_step.py [--batch 32] [--micro 16,8] [--rounds 7] [--out profiles/micro_batch_step.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the benchmark's own model and synthetic batch)
from kai0_amd.config import Pi0Config  # noqa: E402
from kai0_amd.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--micro", default="16,8")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "micro_batch_step.txt"))
ap.add_argument("--commit", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("micro_batch_step.py measures on the GPU; there is none here")

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg, B = Pi0Config(), args.batch
model = bench.build_model(cfg, dev, seed=0)
model.train()
obs, actions = bench.synthetic_batch(cfg, B, seed=1000, device=dev)
trainer = Trainer(model, world_size=1, rank=0, peak_lr=2.5e-5, warmup_steps=1000, decay_steps=30000, end_lr=2.5e-6, weight_decay=1e-10,
                  clip_norm=1.0, mode="zero2", micro_batch=0)  # fmt: skip
assert trainer.micro_batch is None


def one_step(micro):
    trainer.micro_batch = micro
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    trainer.train_step(obs, actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated(dev)


for _ in range(args.warmup):
    one_step(None)
_, peak_unsplit_alone = one_step(None)
variants = [None] + [int(x) for x in args.micro.split(",") if x]
for micro in variants[1:]:  # warm every shape the timed rounds use
    for _ in range(args.warmup):
        one_step(micro)
times, peaks = {v: [] for v in variants}, {v: 0 for v in variants}
for _ in range(args.rounds):
    for micro in variants:
        ms, peak = one_step(micro)
        times[micro].append(ms)
        peaks[micro] = max(peaks[micro], peak)


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


acc_bytes = sum(b.acc.numel() * 4 for b in trainer.engine.buckets if hasattr(b, "acc"))
lines = [f"micro_batch_step probe: B = {B} synthetic (bench.py's model and batch), one GPU, zero2, {args.rounds} alternating rounds after {args.warmup} "
         f"warm-up steps per variant, host clock around a synchronised step; {torch.cuda.get_device_name(0)}; commit {commit()}",
         f"{'variant':<22}{'median ms':>11}{'q1 ms':>9}{'q3 ms':>9}{'IQR ms':>9}{'vs unsplit':>12}{'peak GiB':>10}"]
base = statistics.median(times[None])
for micro in variants:
    q1, q2, q3 = statistics.quantiles(times[micro], n=4)
    name = "unsplit (1 x %d)" % B if micro is None else f"{B // micro} x {micro}"
    lines.append(f"{name:<22}{q2:>11.1f}{q1:>9.1f}{q3:>9.1f}{q3 - q1:>9.1f}{q2 / base:>12.3f}{peaks[micro] / 2**30:>10.2f}")
lines.append(f"peak of the unsplit step before any accumulator existed: {peak_unsplit_alone / 2**30:.2f} GiB; accumulators: {acc_bytes / 2**30:.2f} GiB "
             f"(4 B x {acc_bytes // 4} elements, allocated by the first split step and kept)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
