"""Frames per second of compute_norm_stats' three forms on one synthetic Agilex-shaped dataset (14-column state / action tables,
action_horizon 50, action_dim 32, delta mask (6, -1, 6, -1)), in one process:
  a  device path           tables resident; per key kai0_chunk_stats_moments, host edges, kai0_chunk_stats_hist, host finishing
                           (`norm_stats.device_results`, upload included), and the two "actions" kernels on their own
  b  lowered host path     `norm_stats.host_stats` (chunk_rows in slabs + the one-shot estimator) on a sample of the frames
  c  streamed RunningStats the reference script's update loop alone, 32 frames per update, on transformed rows that already exist
                           (no data loader, no decoding: its floor)
on three tables: a joint-like random walk, the same with two gripper-like two-valued columns, and white noise (no two consecutive
chunk rows share a bin: the histogram kernel's run merging finds nothing to merge — the spread between the tables is the price of the
LDS counter traffic).
With --view, per table, also the two "actions" kernels through the _view entry points, on the resident tables:
  v0  no view               frame_stride = frame_mirror = NULL: the launches of form a, reached through the new entry points
  v1  stride 2 + mirror     the augmented dataset of space_mirror + TimeScaling(2): every second row of every episode, once as it is
                            and once mirrored (`lerobot_dataset.plan_view`) — as many frames as the plain table has rows
usage: python tools/probes/norm_stats_rate.py [--frames N] [--rounds R] [--view] [--out profiles/norm_stats.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kai0_amd import lerobot_dataset as lrd  # noqa: E402
from kai0_amd import norm_stats as ns  # noqa: E402
from kai0_amd.normalize import RunningStats  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2_160_000)
ap.add_argument("--episode", type=int, default=540)
ap.add_argument("--horizon", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-frames", type=int, default=20_000)
ap.add_argument("--streamed-frames", type=int, default=6_400)
ap.add_argument("--view", action="store_true", help="also time the _view entry points: no view, and stride 2 + mirror on half the frames")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_stats.txt"))
ap.add_argument("--commit", default=None, help="commit to record (default: git rev-parse HEAD, 'unknown' outside a git checkout)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("norm_stats_rate.py measures on the GPU; there is none here")

H, D = args.horizon, 14
SPEC = ns.ChunkSpec("observation.state", "action", 32, True, True, False, 0b01111110111111)
n_ep = max(1, args.frames // args.episode)
N = n_ep * args.episode
ep_end = np.repeat(np.arange(1, n_ep + 1) * args.episode, args.episode).astype(np.int32)


def table(kind: str):
    rng = np.random.default_rng(0)
    if kind == "white noise":
        state = rng.uniform(-3, 3, size=(N, D)).astype(np.float32)
        return state, rng.uniform(-3, 3, size=(N, D)).astype(np.float32)
    steps = rng.normal(0, 0.02, size=(n_ep, args.episode + 1, D)).astype(np.float32)
    walk = rng.uniform(-1.5, 1.5, size=(n_ep, 1, D)).astype(np.float32) + np.cumsum(steps, axis=1)
    if kind == "walk + grippers":
        for g in (6, 13):
            walk[:, :, g] = np.where(np.sin(np.arange(args.episode + 1) / 7.0 + g) > 0, 0.07, 0.0)
    state = walk[:, :-1].reshape(N, D)
    action = walk[:, 1:].reshape(N, D) + rng.normal(0, 0.002, size=(N, D)).astype(np.float32)
    if kind == "walk + grippers":
        action[:, [6, 13]] = walk[:, 1:][:, :, [6, 13]].reshape(N, 2)
    return np.ascontiguousarray(state, np.float32), np.ascontiguousarray(action, np.float32)


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


lines = [f"norm_stats probe: N = {N} frames in {n_ep} episodes of {args.episode}, horizon {H}, 14 -> 32 columns ({N * H * 32 / 1e9:.2f} G virtual "
         f"elements per 'actions' key), delta mask (6, -1, 6, -1); {args.rounds} rounds after one warm-up, medians; "
         f"{torch.cuda.get_device_name(0)}; commit {commit()}"]
lines.append(f"{'table / form':<58}{'median s':>11}{'min s':>10}{'frames/s':>14}")
dev = torch.device("cuda:0")
kw = dict(horizon=H, width=32, clip_state=True, clip_action=True, mask_state=False, delta_mask=SPEC.delta_mask)
for kind in ("walk", "walk + grippers", "white noise"):
    state, action = table(kind)
    t_state, t_action, t_end = (torch.from_numpy(x).to(dev) for x in (state, action, ep_end))
    whole, mom, hist = [], [], []
    for r in range(args.rounds + 1):
        t, res = timed(lambda: ns.device_results(state, action, ep_end, SPEC, H))
        t1, sums = timed(lambda: ns.device_sums(t_state, t_action, t_end, None, **kw))
        edges = np.stack([ns.column_edges(sums.lo[c], sums.hi[c]) for c in range(32)])
        mask = sum(1 << c for c in range(32) if sums.lo[c] != sums.hi[c])
        t2, _ = timed(lambda: ns.device_hist(t_state, t_action, t_end, None, edges, mask, **kw))
        if r:
            whole.append(t), mom.append(t1), hist.append(t2)
    for name, ts in (("a  device path, both keys, upload + finishing", whole), ("   kai0_chunk_stats_moments ('actions')", mom),
                     (f"   kai0_chunk_stats_hist ('actions', {bin(mask).count('1')} columns)", hist)):  # fmt: skip
        m = statistics.median(ts)
        label = kind + ": " + name
        lines.append(f"{label:<58}{m:>11.4f}{min(ts):>10.4f}{N / m:>14.3e}")
    if args.view:
        plan = lrd.plan_view([args.episode] * n_ep, None, lrd.TimeScaling(2), True)
        t_plan = tuple(torch.from_numpy(x).to(dev) for x in (plan.frame_idx, plan.frame_stride, plan.frame_mirror))
        forms = (("v0 no view (NULL, NULL)", None, (None, None, 7, 7)),
                 (f"v1 stride 2 + mirror on half, {len(plan)} frames", t_plan[0], (t_plan[1], t_plan[2], 7, 7)))  # fmt: skip
        for label, t_idx, view in forms:
            m = N if t_idx is None else len(plan)
            mom, hist = [], []
            for r in range(args.rounds + 1):
                t1, sums = timed(lambda: ns.device_sums(t_state, t_action, t_end, t_idx, **kw, view=view))
                edges = np.stack([ns.column_edges(sums.lo[c], sums.hi[c]) for c in range(32)])
                mask = sum(1 << c for c in range(32) if sums.lo[c] != sums.hi[c])
                t2, _ = timed(lambda: ns.device_hist(t_state, t_action, t_end, t_idx, edges, mask, **kw, view=view))
                if r:
                    mom.append(t1), hist.append(t2)
            for name, ts in (("kai0_chunk_stats_moments_view", mom), ("kai0_chunk_stats_hist_view", hist)):
                med = statistics.median(ts)
                line = f"{kind}: {label}: {name}"
                lines.append(f"{line:<96}{med:>11.4f}{min(ts):>10.4f}{m / med:>14.3e}")
    if kind == "walk + grippers":
        idx = np.sort(np.random.default_rng(0).choice(N, size=min(N, args.host_frames), replace=False))
        t0 = time.perf_counter()
        host = ns.host_stats(state, action, ep_end, SPEC, H, idx)
        tb = time.perf_counter() - t0
        label = f"{kind}: b  lowered host path, {len(idx)} frames"
        lines.append(f"{label:<58}{tb:>11.4f}{'':>10}{len(idx) / tb:>14.3e}")
        ms = min(N, args.streamed_frames)
        rows_s, rows_a = ns.chunk_rows(state, action, ep_end, horizon=H, action_dim=32, clip_state=True, clip_action=True, mask_state=False,
                                       delta_mask=SPEC.delta_mask, frame_idx=np.arange(ms))  # fmt: skip
        t0 = time.perf_counter()
        rs = {"state": RunningStats(), "actions": RunningStats()}
        for i in range(0, ms, 32):
            rs["state"].update(rows_s[i : i + 32])
            rs["actions"].update(rows_a[i : i + 32])
        tc = time.perf_counter() - t0
        label = f"{kind}: c  streamed RunningStats(32), {ms} frames"
        lines.append(f"{label:<58}{tc:>11.4f}{'':>10}{ms / tc:>14.3e}")
        sub = ns.device_results(state, action, ep_end, SPEC, H, idx)
        same = all(np.array_equal(getattr(sub[k].stats, f), getattr(host[k], f)) for k in ns.KEYS for f in ("q01", "q99"))
        lines.append(f"agreement on that sample: device q01 / q99 == host q01 / q99: {same}; max |mean difference| "
                     f"{max(float(np.abs(sub[k].stats.mean - host[k].mean).max()) for k in ns.KEYS):.3e}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
