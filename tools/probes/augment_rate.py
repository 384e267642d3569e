"""Milliseconds per step of the train-time image augmentation alone, in its two forms, in one process:
  batch       the torch port's one draw per camera and call (`preprocessing._augment`: about 20 torch kernels per geometric camera)
  per_sample  one draw per sample, applied by csrc/augment.hip (`ops.augment_images`: two launches per camera, one host-to-device copy
              of all cameras' parameters per call)
on the trainer's per-rank batch: B = 32, three 224 x 224 cameras, `--geometric` of them (default 2) with the crop and the rotation and
the others colour only (the model's own camera set, one base and two wrist cameras, is `--geometric 1`), f32 NCHW on the device.
Each step is `preprocess_observation(train=True, augment=...)` — host draws included — between two device events; the forms alternate
step by step; medians after a warm-up.  The device kernels and copies each form enqueues per step are counted in a
separate, profiled step (torch.profiler), not in the timed ones.
usage: python tools/probes/augment_rate.py [--geometric 2] [--batch 32] [--steps 30] [--warmup 5] [--out profiles/augment_rate.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kai0_amd import preprocessing as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--res", type=int, default=224)
ap.add_argument("--geometric", type=int, default=2, choices=(0, 1, 2, 3), help="how many of the three cameras are geometric")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_rate.txt"))
ap.add_argument("--commit", default=None, help="commit to record (default: git rev-parse HEAD, 'unknown' outside a git checkout)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("augment_rate.py measures on the GPU; there is none here")
if args.steps < 20:
    sys.exit("augment_rate.py: at least 20 timed steps")

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
KEYS = [f"base_{i}_rgb" if i < args.geometric else f"left_wrist_{i}_rgb" for i in range(3)]  # "wrist" in the key: colour only
images = {k: (torch.rand(args.batch, 3, args.res, args.res, generator=g) * 2 - 1).to(dev) for k in KEYS}
obs = types.SimpleNamespace(images=images, image_masks={}, state=torch.zeros(args.batch, 32, device=dev), tokenized_prompt=None,
                            tokenized_prompt_mask=None)  # fmt: skip
MODES = ("batch", "per_sample")


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def step(mode):
    return P.preprocess_observation(obs, train=True, image_keys=KEYS, augment=mode)


def device_ops(mode):
    """(kernels, copies) one step enqueues, from a profiled step of its own; None where the profiler reports no device activity."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step(mode)
        torch.cuda.synchronize()
    on_device = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not on_device:
        return None
    copies = sum(1 for e in on_device if "memcpy" in e.name.lower() or "memset" in e.name.lower())
    return len(on_device) - copies, copies


torch.manual_seed(0)
times = {m: [] for m in MODES}
for i in range(args.warmup + args.steps):
    for mode in MODES:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        step(mode)
        end.record()
        end.synchronize()
        if i >= args.warmup:
            times[mode].append(start.elapsed_time(end))
counts = {}
for mode in MODES:
    try:
        counts[mode] = device_ops(mode)
    except Exception as exc:  # the profiler is an optional part of the report; the timings above do not depend on it
        counts[mode] = None
        print(f"launch count of {mode!r} not measured: {type(exc).__name__}: {exc}")

lines = [f"augmentation probe: B = {args.batch}, three {args.res} x {args.res} cameras ({args.geometric} geometric, the others colour only), f32 NCHW; "
         f"{args.steps} steps after {args.warmup} warm-up, forms alternating, device events around preprocess_observation(train=True); "
         f"{torch.cuda.get_device_name(0)}; commit {commit()}"]  # fmt: skip
lines.append(f"{'form':<12}{'median ms':>11}{'min ms':>9}{'max ms':>9}{'kernels / step':>17}{'copies / step':>16}")
for mode in MODES:
    ts = times[mode]
    k, c = counts[mode] if counts[mode] else ("not measured", "not measured")
    lines.append(f"{mode:<12}{statistics.median(ts):>11.3f}{min(ts):>9.3f}{max(ts):>9.3f}{k!s:>17}{c!s:>16}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
