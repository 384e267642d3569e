"""Streaming rate of kai0_grad_accum beside kai0_adamw_ema on ONE 256 Mi-element shard (bf16 gradient), in one process, warmed up,
then alternated a, b, c, d, a, b, ... with device events around each call; median and interquartile range per variant.
  a  kai0_adamw_ema                      36 B per element (master, two moments and EMA read + written, bf16 gradient read, bf16 model copy written)
  b  kai0_grad_accum first=0             10 B (bf16 gradient read, f32 accumulator read + written)
  c  kai0_grad_accum first=0 + sumsq_out 10 B, plus the 4096 partials and the finishing launch
  d  kai0_grad_accum first=1              6 B (the accumulator is not read)
usage: python tools/probes/grad_accum.py [--elements N] [--rounds R] [--out profiles/grad_accum.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kai0_amd import optim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=256 << 20)
ap.add_argument("--rounds", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_accum.txt"))
ap.add_argument("--commit", default=None, help="commit to record (default: git rev-parse HEAD, 'unknown' outside a git checkout)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("grad_accum.py measures on the GPU; there is none here")

dev = torch.device("cuda:0")
n, D = args.elements, 0.99
BF16 = torch.bfloat16
master = torch.randn(n, device=dev) * 0.02
m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
ema = master.clone()
grad = (torch.randn(n, device=dev) * 1e-2).to(BF16)
param = master.to(BF16)
acc = torch.zeros(n, device=dev)
sumsq = torch.zeros(1, device=dev)
kw = dict(lr=2.5e-5, beta1=0.9, beta2=0.95, eps=1e-8, wd=1e-10, clip_coef=torch.ones(1, device=dev))
step = [0]


def a():
    optim.adamw_step_(master, m, v, grad, param, step=step[0], ema=ema, ema_decay=D, **kw)


def b():
    optim.grad_accum_(acc, grad, first=False)


def c():
    optim.grad_accum_(acc, grad, first=False, sumsq_out=sumsq)


def d():
    optim.grad_accum_(acc, grad, first=True)


variants = [("a  kai0_adamw_ema", a, 36), ("b  grad_accum", b, 10), ("c  grad_accum + sumsq", c, 10), ("d  grad_accum first", d, 6)]
times = {name: [] for name, _, _ in variants}
for r in range(args.warmup + args.rounds):
    step[0] += 1
    for name, fn, _ in variants:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if r >= args.warmup:
            times[name].append(s.elapsed_time(e))


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


rate, lines = {}, []
lines.append(f"grad_accum probe: {n} elements ({n / 2**20:.0f} Mi), bf16 gradient, {args.rounds} alternating rounds after {args.warmup} warm-up "
             f"rounds, device events per call; {torch.cuda.get_device_name(0)}; commit {commit()}")
lines.append(f"{'variant':<28}{'median ms':>11}{'q1 ms':>9}{'q3 ms':>9}{'IQR ms':>9}{'B/elem':>8}{'GB/s':>9}")
for name, _, nbytes in variants:
    q1, q2, q3 = statistics.quantiles(times[name], n=4)
    rate[name[0]] = n * nbytes / q2 / 1e6
    lines.append(f"{name:<28}{q2:>11.3f}{q1:>9.3f}{q3:>9.3f}{q3 - q1:>9.3f}{nbytes:>8}{rate[name[0]]:>9.0f}")
lines.append(f"GB/s relative to kai0_adamw_ema: b {rate['b'] / rate['a']:.3f}, c {rate['c'] / rate['a']:.3f}, d {rate['d'] / rate['a']:.3f}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
