"""LoRA on the HIP path, measured in ONE process, warmed up, variants alternated round by round, device events around each call; median
and interquartile range per variant (the pattern of tools/probes/grad_accum.py).

(a) kernels — kai0_lora_down and kai0_lora_wgrad on their production shapes (M = 30976 = 32 x 968 PaliGemma rows with K or C in
    {2048, 16384}, R in {16, 32}; M = 1600 = 32 x 50 expert rows with {1024, 4096}, R in {32, 64}), next to kai0_gemm_bf16 through
    ops.gemm on the identical operands with the split the existing rules choose (ops.pick_split_k for the NT down-projection,
    ops.pick_split_k_wgrad for the TN gradient), in GB/s of algorithmic bytes (every operand and the result once).  Operands are
    rotated over enough copies that no call finds its activation in the 256 MiB Infinity Cache.  The record ends with the dispatch
    rule the numbers give: a shape whose new kernel does not beat ops.gemm by more than the interquartile range goes to ops.gemm.
(b) step — the full-size pi0.5 LoRA step (gemma_2b_lora + gemma_300m_lora, towers frozen per Pi0Config.get_freeze_filter) next to
    the full fine-tune step of the same build, bench.py's model and synthetic batch: ms per step, samples/s and
    torch.cuda.max_memory_allocated of each.  (--trace-steps N runs N steps of --trace-mode and exits: the target of a
    `rocprofv3 --kernel-trace` run whose database tools/step_anatomy.py breaks down by kernel family.)
usage: python tools/probes/lora.py [--part a|b|ab] [--batch 32] [--rounds 30] [--step-rounds 7] [--out profiles/lora.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kai0_amd import _lib, lora, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="ab")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--step-rounds", type=int, default=7)
ap.add_argument("--trace-steps", type=int, default=0)
ap.add_argument("--trace-mode", default="lora", choices=["lora", "full"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora.txt"))
ap.add_argument("--commit", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("lora.py measures on the GPU; there is none here")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
BF16 = torch.bfloat16


def commit():
    if args.commit:
        return args.commit
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def quart(xs):
    q1, q2, q3 = statistics.quantiles(xs, n=4)
    return q1, q2, q3


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def copies(nbytes):
    return max(2, -(-(600 << 20) // nbytes))  # the rotation covers > 2 x the Infinity Cache


def kernels_part():
    lines = [f"{'kernel':<10}{'M':>7}{'K|C':>7}{'R':>4} | {'new us':>9}{'IQR':>7}{'GB/s':>7} | {'ops.gemm us':>12}{'IQR':>7}{'GB/s':>7}{'split':>6} | use"]
    rule = {"down": [], "wgrad": []}
    shapes = [(30976, w, r) for w in (2048, 16384) for r in (16, 32)] + [(1600, w, r) for w in (1024, 4096) for r in (32, 64)]
    for kind in ("down", "wgrad"):
        for M, W, R in shapes:
            n = copies(M * W * 2)
            xs = [torch.randn(M, W, device=dev, dtype=BF16) for _ in range(n)]
            if kind == "down":  # T = X A^T
                a = torch.randn(R, W, device=dev, dtype=BF16) * 0.05
                out = torch.empty(M, R, device=dev, dtype=BF16)
                split = ops.pick_split_k(M, R, W)
                new = lambda i: _lib.call("kai0_lora_down", xs[i % n].data_ptr(), W, a.data_ptr(), W, out.data_ptr(), R, M, R, W, ops._stream())  # noqa: E731
                old = lambda i: ops.gemm(xs[i % n], a, out, M=M, N=R, K=W, lda=W, ldb=W, ldc=R, split_k=split)  # noqa: E731
                nbytes = 2 * (M * W + R * W + M * R)
            else:  # G = P^T Q, P [M, R], Q = X [M, C]
                p = torch.randn(M, R, device=dev, dtype=BF16)
                out = torch.empty(R, W, device=dev, dtype=BF16)
                split = ops.pick_split_k_wgrad(R, W, M)
                new = lambda i: lora.lora_wgrad(p, xs[i % n], out, M=M, R=R, C=W, ldp=R, ldq=W, ldg=W)  # noqa: E731
                old = lambda i: ops.gemm(p, xs[i % n], out, M=R, N=W, K=M, a_kc=False, b_kc=False, lda=R, ldb=W, ldc=W, split_k=split)  # noqa: E731
                nbytes = 2 * (M * W + M * R + R * W)
            t = {"new": [], "old": []}
            for r in range(args.warmup + args.rounds):
                for name, fn in (("new", new), ("old", old)):
                    ms = timed(lambda: fn(r))
                    if r >= args.warmup:
                        t[name].append(ms * 1e3)
            (n1, n2, n3), (o1, o2, o3) = quart(t["new"]), quart(t["old"])
            use = "new" if n2 < o2 - max(n3 - n1, o3 - o1) else "ops.gemm"
            rule[kind].append(((M, W, R), use))
            lines.append(f"{kind:<10}{M:>7}{W:>7}{R:>4} | {n2:>9.1f}{n3 - n1:>7.1f}{nbytes / n2 / 1e3:>7.0f} | {o2:>12.1f}{o3 - o1:>7.1f}"
                         f"{nbytes / o2 / 1e3:>7.0f}{split:>6} | {use}")
            del xs
            torch.cuda.empty_cache()
    for kind, rs in rule.items():
        lost = [s for s, u in rs if u != "new"]
        lines.append(f"dispatch rule, {kind}: " + ("the new kernel on every measured shape" if not lost else
                                                   f"ops.gemm on (M, K|C, R) = {lost}, the new kernel elsewhere"))
    return lines


def step_part():
    import bench
    from kai0_amd.config import Pi0Config
    from kai0_amd.train import Trainer, apply_freeze_filter

    B = args.batch
    cfgs = {"full": Pi0Config(), "lora": Pi0Config(paligemma_variant="gemma_2b_lora", action_expert_variant="gemma_300m_lora")}
    modes = [args.trace_mode] if args.trace_steps else ["full", "lora"]
    tr, batch = {}, {}
    for name in modes:
        cfg = cfgs[name]
        model = bench.build_model(cfg, dev, seed=0)
        model.train()
        frozen = apply_freeze_filter(model, cfg.get_freeze_filter())
        tr[name] = (Trainer(model, world_size=1, rank=0, peak_lr=2.5e-5, warmup_steps=1000, decay_steps=30000, end_lr=2.5e-6,
                            weight_decay=1e-10, clip_norm=1.0, mode="zero2", micro_batch=0), frozen,
                    sum(p.numel() for p in model.parameters() if p.requires_grad))  # fmt: skip
        batch[name] = bench.synthetic_batch(cfg, B, seed=1000, device=dev)

    def one(name):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        tr[name][0].train_step(*batch[name])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated(dev)

    if args.trace_steps:
        for _ in range(args.trace_steps):
            one(args.trace_mode)
        sys.exit(0)
    for name in modes:
        for _ in range(2):
            one(name)
    times, peaks = {n: [] for n in modes}, {n: 0 for n in modes}
    for _ in range(args.step_rounds):
        for name in modes:
            ms, pk = one(name)
            times[name].append(ms)
            peaks[name] = max(peaks[name], pk)
    lines = [f"step at B = {B} (bench.py's model and synthetic batch, one GPU, zero2, both models resident in the process; {args.step_rounds} "
             "alternating rounds after 2 warm-up steps each, host clock around a synchronised step)",
             f"{'variant':<18}{'median ms':>11}{'q1':>9}{'q3':>9}{'IQR':>8}{'samples/s':>11}{'peak GiB':>10}{'trained M':>11}{'frozen M':>10}"]
    for name in modes:
        q1, q2, q3 = quart(times[name])
        lines.append(f"{name:<18}{q2:>11.1f}{q1:>9.1f}{q3:>9.1f}{q3 - q1:>8.1f}{B / q2 * 1e3:>11.1f}{peaks[name] / 2**30:>10.2f}"
                     f"{tr[name][2] / 1e6:>11.1f}{tr[name][1] / 1e6:>10.1f}")
    lines.append("(the peak of a variant includes the other model's resident weights and optimizer state: compare the difference, "
                 f"full - lora = {(peaks['full'] - peaks['lora']) / 2**30:.2f} GiB, not the absolute values)")
    lines.append(f"lora / full step time: {statistics.median(times['lora']) / statistics.median(times['full']):.3f}")
    return lines


text = [f"lora probe: {torch.cuda.get_device_name(0)}; commit {commit()}; {args.rounds} alternating rounds after {args.warmup} warm-up rounds, "
        "device events per call"]
if "a" in args.part and not args.trace_steps:
    text += kernels_part()
if "b" in args.part or args.trace_steps:
    text += step_part()
out = "\n".join(text) + "\n"
print(out, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(out)
