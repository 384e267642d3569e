"""Frames per second of Stage-Advantage annotation (two-timestep mode) on one GPU, the full-size estimator on synthetic weights, one
synthetic episode of 480 x 640 uint8 frames:
  a  the evaluator's way   per batch: every current and future image prepared on host threads as f32 (`_process_single_image`, the
                           next batch prefetched while the GPU works), uploaded as f32, frame 0 expanded to the batch, then two
                           `AdvantageEstimator.sample_values` calls on six-image observations with the 200-slot prompt
                           (stage_advantage/annotation/evaluator.py:249-484) — the only path before kai0_amd.stage_advantage
  b  ValueAnnotator        uint8 upload, kai0_frames_to_chw, every image through SigLIP once into the ring bank, kai0_prefix_gather,
                           the prompt trimmed to its valid length rounded up to 8, both passes as one batch
Both get the same injected noise and time, so their values are comparable: the largest |difference| is reported.  Each variant runs
`--warmup` frames first (kernel selection, allocator), then the episode `--rounds` times, alternating; wall clock around a
synchronised episode, median reported.
usage: python tools/probes/annotate_rate.py [--frames 64] [--interval 50] [--batch-size 16] [--out profiles/stage_advantage_rate.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time as clock
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kai0_amd.config import AdvantageEstimatorConfig  # noqa: E402
from kai0_amd.model import AdvantageEstimator  # noqa: E402
from kai0_amd.preprocessing import resize_with_pad_torch  # noqa: E402
from kai0_amd.stage_advantage import ValueAnnotator, advantages_from_values  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--interval", type=int, default=50)
ap.add_argument("--batch-size", type=int, default=16)
ap.add_argument("--siglip-batch", type=int, default=96)
ap.add_argument("--valid-tokens", type=int, default=10, help="'Flatten and fold the cloth.' is about 10 tokens of the 200 slots")
ap.add_argument("--workers", type=int, default=16)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=16, help="frames of the warm-up episode")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_advantage_rate.txt"))
ap.add_argument("--commit", default=None, help="commit to record (default: git rev-parse HEAD, 'unknown' outside a git checkout)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("annotate_rate.py measures on the GPU; there is none here")

dev = torch.device("cuda:0")
torch.manual_seed(1)
with torch.device(dev):
    model = AdvantageEstimator(AdvantageEstimatorConfig(loss_value_weight=1.0, loss_action_weight=0.0))
with torch.no_grad():
    for k, p in model.named_parameters():
        if "dense.weight" in k:
            p.normal_(0.0, 0.02)
model.eval()
cfg = model.config
T, Hs, A = cfg.max_token_len, cfg.action_horizon, cfg.action_dim
rng = np.random.default_rng(0)
tokens = np.zeros(T, dtype=np.int64)
tokens[: args.valid_tokens] = rng.integers(1, 2048, args.valid_tokens)
mask = np.arange(T) < args.valid_tokens
pool = ThreadPoolExecutor(max_workers=args.workers)


def episode(F):
    g = np.random.default_rng(F)
    frames = [g.integers(0, 256, size=(F, 480, 640, 3), dtype=np.uint8) for _ in range(3)]
    tg = torch.Generator().manual_seed(F)
    return frames, torch.randn((2, F, Hs, A), generator=tg), torch.rand((2, F), generator=tg) * 0.999 + 0.001


def process_single_image(rgb):  # evaluator.py:151-165
    t = torch.from_numpy(rgb).float() / 255.0
    t = t * 2.0 - 1.0
    return resize_with_pad_torch(t, 224, 224)[0].permute(2, 0, 1)


def evaluator_way(frames, noise, time):
    F, B, D = frames[0].shape[0], args.batch_size, args.interval
    initial = [process_single_image(f[0])[None].to(dev) for f in frames]
    tok = torch.from_numpy(tokens)
    msk = torch.from_numpy(mask)
    starts = list(range(0, F, B))

    def prepare(s):
        idx = list(range(s, min(s + B, F)))
        fut = [min(j + D, F - 1) for j in idx]
        tensors = list(pool.map(process_single_image, [f[j] for j in idx + fut for f in frames]))
        n = len(idx)
        return [torch.stack(tensors[c : 3 * n : 3]) for c in range(3)], [torch.stack(tensors[3 * n + c :: 3]) for c in range(3)], idx

    raw = torch.zeros((2, F))
    nxt = pool.submit(prepare, starts[0])
    for k, s in enumerate(starts):
        base, future, idx = nxt.result()
        if k + 1 < len(starts):
            nxt = pool.submit(prepare, starts[k + 1])
        n = len(idx)
        base, future = [t.to(dev) for t in base], [t.to(dev) for t in future]
        names = ("base", "left_wrist", "right_wrist")
        common = dict(state=torch.zeros((n, 32), device=dev), image_masks={}, tokenized_prompt=tok[None].expand(n, -1).contiguous().to(dev),
                      tokenized_prompt_mask=msk[None].expand(n, -1).contiguous().to(dev))  # fmt: skip
        rel = SimpleNamespace(images={**{f"{p}_-100_rgb": base[c] for c, p in enumerate(names)},
                                      **{f"{p}_0_rgb": future[c] for c, p in enumerate(names)}}, **common)  # fmt: skip
        ab = SimpleNamespace(images={**{f"{p}_-100_rgb": initial[c].expand(n, -1, -1, -1) for c, p in enumerate(names)},
                                     **{f"{p}_0_rgb": base[c] for c, p in enumerate(names)}}, **common)  # fmt: skip
        for p, obs in ((0, rel), (1, ab)):
            v = model.sample_values(dev, obs, noise=noise[p, idx[0] : idx[-1] + 1].to(dev), time=time[p, idx[0] : idx[-1] + 1].to(dev))
            raw[p, idx[0] : idx[-1] + 1] = v.reshape(-1).cpu()
    return raw.numpy()


annotator = ValueAnnotator(model, batch_size=args.batch_size, siglip_batch=args.siglip_batch, trim_prompt=True)


def native_way(frames, noise, time):
    out = annotator.annotate(frames, tokens, mask, relative_interval=args.interval, noise=noise, time=time)
    return np.stack([out["raw_relative"], out["raw_absolute"]])


variants = [("a  evaluator's way", evaluator_way), ("b  ValueAnnotator", native_way)]
warm = episode(args.warmup)
for _, fn in variants:
    fn(*warm)
ep = episode(args.frames)
times = {name: [] for name, _ in variants}
values = {}
for _ in range(args.rounds):
    for name, fn in variants:
        torch.cuda.synchronize()
        t0 = clock.perf_counter()
        values[name] = fn(*ep)
        torch.cuda.synchronize()
        times[name].append(clock.perf_counter() - t0)
pool.shutdown()
va, vb = (values[name] for name, _ in variants)
diff = float(np.abs(va - vb).max())
adv = advantages_from_values(vb[1], vb[0], relative_interval=args.interval)


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


lines = [f"annotate_rate probe: full-size AdvantageEstimator (synthetic weights), {args.frames} synthetic 480x640 frames x 3 cameras, two-timestep "
         f"mode, relative_interval {args.interval}, batch {args.batch_size}, prompt {args.valid_tokens} valid tokens of {T}; {args.rounds} alternating "
         f"episodes after a {args.warmup}-frame warm-up, wall clock per synchronised episode; {torch.cuda.get_device_name(0)}; commit {commit()}",
         f"{'variant':<24}{'median s':>10}{'min s':>9}{'max s':>9}{'frames/s':>10}"]  # fmt: skip
med = {}
for name, _ in variants:
    med[name[0]] = statistics.median(times[name])
    lines.append(f"{name:<24}{med[name[0]]:>10.3f}{min(times[name]):>9.3f}{max(times[name]):>9.3f}{args.frames / med[name[0]]:>10.2f}")
lines.append(f"time of the evaluator's way / time of ValueAnnotator: {med['a'] / med['b']:.2f} x; images through SigLIP per episode: "
             f"{3 * args.frames} (b) vs {3 + 12 * args.frames} (a)")
lines.append(f"agreement: largest |value(a) - value(b)| over both passes {diff:.3e}; |advantage| <= {float(np.abs(adv['absolute_advantage']).max()):.3f}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
