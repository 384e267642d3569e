"""Streaming rate of kai0_mix and kai0_multi_dot beside the torch-op forms they replace, on N resident bf16 checkpoints of one 256 Mi-element
tensor, in one process, warmed up, then alternated a, b, c, d, a, b, ... with device events around each call; median and interquartile
range per variant.
  a  kai0_mix                        N x 2 B read + 2 B written per element
  b  torch mix                       the reference loop's ops on device-resident tensors: sum(w[i] * src[i] for i in range(N)) —
                                     N multiplies and N - 1 adds, each a pass of its own with a temporary (arithmetic_torch.py:190-195)
  c  kai0_multi_dot                  (N + 1) x 2 B read per element, one pass; the finishing launch included
  d  torch projection                (g * src[i]).sum() per source, kept on the device (arithmetic_torch.py:210-214 without .item())
The implied bytes/s of a and c stand against the 5-6 TB/s kai0_adamw reaches.
usage: python tools/probes/model_arithmetic.py [--elements N] [--sources N] [--rounds R] [--out profiles/model_arithmetic.txt]"""
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
ap.add_argument("--sources", type=int, default=4)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_arithmetic.txt"))
ap.add_argument("--commit", default=None, help="commit to record (default: git rev-parse HEAD, 'unknown' outside a git checkout)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("model_arithmetic.py measures on the GPU; there is none here")

dev = torch.device("cuda:0")
n, N = args.elements, args.sources
BF16 = torch.bfloat16
gen = torch.Generator(device=dev).manual_seed(0)
srcs = [(torch.randn(n, device=dev, generator=gen) * 0.02).to(BF16) for _ in range(N)]
grad = (torch.randn(n, device=dev, generator=gen) * 1e-2).to(BF16)
dst = torch.empty(n, device=dev, dtype=BF16)
w = torch.softmax(torch.arange(N, dtype=torch.float64) * 0.3, 0)
w_host = w.tolist()
w_dev = w.to(torch.float32).to(dev)
out = torch.zeros(N, dtype=torch.float64, device=dev)
keep = {}


def a():
    optim.mix_(dst, srcs, w_host)


def b():
    keep["mixed"] = sum(w_dev[i] * srcs[i] for i in range(N))


def c():
    out.zero_()
    optim.multi_dot_(grad, srcs, out)


def d():
    keep["g"] = [(grad * srcs[i]).sum() for i in range(N)]


variants = [("a  kai0_mix", a, 2 * N + 2), ("b  torch mix", b, None), ("c  kai0_multi_dot", c, 2 * N + 2), ("d  torch projection", d, None)]
times = {name: [] for name, _, _ in variants}
for r in range(args.warmup + args.rounds):
    for name, fn, _ in variants:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        if r >= args.warmup:
            times[name].append(s.elapsed_time(e))

# the two forms agree: the torch mix rounds every product and sum to bf16, the kernel once; the projections differ by summation order
mix_diff = float((dst.float() - keep["mixed"].float()).abs().max())
proj_rel = max(abs(float(out[i]) - float(keep["g"][i].double())) / (abs(float(out[i])) + 1e-30) for i in range(N))


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


med, lines = {}, []
lines.append(f"model_arithmetic probe: {N} bf16 sources of {n} elements ({n / 2**20:.0f} Mi), bf16 gradient and destination, {args.rounds} alternating "
             f"rounds after {args.warmup} warm-up rounds, device events per call; {torch.cuda.get_device_name(0)}; commit {commit()}")
lines.append(f"{'variant':<28}{'median ms':>11}{'q1 ms':>9}{'q3 ms':>9}{'IQR ms':>9}{'B/elem':>8}{'GB/s':>9}")
for name, _, nbytes in variants:
    q1, q2, q3 = statistics.quantiles(times[name], n=4)
    med[name[0]] = q2
    tail = f"{nbytes:>8}{n * nbytes / q2 / 1e6:>9.0f}" if nbytes else f"{'-':>8}{'-':>9}"
    lines.append(f"{name:<28}{q2:>11.3f}{q1:>9.3f}{q3:>9.3f}{q3 - q1:>9.3f}{tail}")
lines.append(f"time of the torch-op form / time of the kernel: mix {med['b'] / med['a']:.2f} x, projection {med['d'] / med['c']:.2f} x")
lines.append(f"agreement: max |kai0_mix - torch mix| {mix_diff:.3e} (bf16 tensors of scale 0.02; torch rounds every op to bf16), "
             f"projection relative difference {proj_rel:.3e}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
