"""What the parameter EMA costs inside the AdamW pass: (a) kai0_adamw, (b) kai0_adamw_ema, (c) kai0_adamw followed by
`ema.lerp_(master, 1 - d)` on ONE 256 Mi-element shard (bf16 gradient and model copy: 5.4 GB of buffers, the size of a real bucket's
shard on one GPU), in one process, warmed up, then alternated a, b, c, a, b, c, ... with device events around each; median and
interquartile range per variant.  Algorithmic bytes per element: (a) 28, (b) 36, (c) 40.
The non-finite guard adds four columns: the tail of the optimizer step as the engine launches it, clip coefficient
then update, unguarded and guarded — (d) kai0_clip_coef + kai0_adamw_ema against (e) kai0_clip_coef_guard + kai0_adamw_ema on the same
shard, and (f) / (g) the same pair around kai0_adamw_rows_ema at the embedding table's shape (257152 x 2048, bf16 gradient with
`--touched` nonzero rows: an idle row costs its gradient read).  To
compare two builds of the library run the probe once per build (KAI0_HIP_LIB selects it), alternating, and compare (b), (d), (f).
usage: python tools/probes/ema_adamw.py [--elements N] [--rounds R] [--out profiles/ema_adamw.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_adamw.txt"))
ap.add_argument("--rows", type=int, default=257152, help="rows of the row-sparse case (0: leave (f), (g) out)")
ap.add_argument("--row-len", type=int, default=2048)
ap.add_argument("--touched", type=int, default=6400, help="rows with a nonzero gradient (a step touches at most B x 200)")
ap.add_argument("--commit", default=None, help="commit to record (default: git rev-parse HEAD, 'unknown' outside a git checkout)")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ema_adamw.py measures on the GPU; there is none here")

dev = torch.device("cuda:0")
n, D = args.elements, 0.99
BF16 = torch.bfloat16
master = torch.randn(n, device=dev) * 0.02
m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
ema = master.clone()
grad = (torch.randn(n, device=dev) * 1e-2).to(BF16)
param = master.to(BF16)
kw = dict(lr=2.5e-5, beta1=0.9, beta2=0.95, eps=1e-8, wd=1e-10, clip_coef=torch.ones(1, device=dev))
step = [0]


def a():
    optim.adamw_step_(master, m, v, grad, param, step=step[0], **kw)


def b():
    optim.adamw_step_(master, m, v, grad, param, step=step[0], ema=ema, ema_decay=D, **kw)


def c():
    optim.adamw_step_(master, m, v, grad, param, step=step[0], **kw)
    ema.lerp_(master, 1.0 - D)


# ---- the guarded step's tail: the clip coefficient from a finite sum of squares (coef = 1), unguarded and guarded
sumsq, norm = torch.full((1,), 0.25, device=dev), torch.zeros(1, device=dev)
skipped = torch.zeros(1, dtype=torch.int32, device=dev)
kwc = dict(kw, clip_coef=torch.ones(1, device=dev))


def clip(guard):
    if guard:
        optim.clip_coef_guard_(sumsq, 1.0, kwc["clip_coef"], norm, skipped)
    else:
        optim.clip_coef_(sumsq, 1.0, kwc["clip_coef"], norm)


def dense_tail(guard):
    clip(guard)
    optim.adamw_step_(master, m, v, grad, param, step=step[0], ema=ema, ema_decay=D, **kwc)


variants = [("a  kai0_adamw", a, 28), ("b  kai0_adamw_ema", b, 36), ("c  kai0_adamw + ema.lerp_", c, 40),
            ("d  clip_coef + adamw_ema", lambda: dense_tail(False), 36), ("e  clip_coef_guard + adamw_ema", lambda: dense_tail(True), 36)]
if args.rows:
    R, L = args.rows, args.row_len
    r_master = torch.randn(R * L, device=dev) * 0.02
    r_m, r_v, r_ema = torch.zeros(R * L, device=dev), torch.zeros(R * L, device=dev), r_master.clone()
    r_grad = torch.zeros(R, L, dtype=BF16, device=dev)
    r_grad[torch.randperm(R, device=dev)[: args.touched]] = 0.01
    r_grad, r_param = r_grad.reshape(-1), r_master.to(BF16)
    r_active = torch.zeros(R, dtype=torch.uint8, device=dev)
    row_bytes = (2 * R * L + 34 * args.touched * L) / (R * L)  # every row's gradient read + 34 B more per element of a live row

    def rows_tail(guard):
        clip(guard)
        optim.adamw_step_(r_master, r_m, r_v, r_grad, r_param, step=step[0], ema=r_ema, ema_decay=D, row_len=L, row_active=r_active, **kwc)

    variants.append(("f  clip_coef + adamw_rows_ema", lambda: rows_tail(False), row_bytes))
    variants.append(("g  clip_coef_guard + rows_ema", lambda: rows_tail(True), row_bytes))
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


med, lines = {}, []
lines.append(f"ema_adamw probe: {n} elements ({n / 2**20:.0f} Mi), bf16 grad + bf16 model copy, decay {D}, {args.rounds} alternating rounds "
             f"after {args.warmup} warm-up rounds, device events per call; {torch.cuda.get_device_name(0)}; commit {commit()}")
lines.append(f"{'variant':<32}{'median ms':>11}{'q1 ms':>9}{'q3 ms':>9}{'IQR ms':>9}{'B/elem':>8}{'GB/s':>9}")
for name, _, nbytes in variants:
    q1, q2, q3 = statistics.quantiles(times[name], n=4)
    med[name[0]] = (q2, q3 - q1)
    elems = args.rows * args.row_len if name[0] in "fg" else n
    lines.append(f"{name:<32}{q2:>11.3f}{q1:>9.3f}{q3:>9.3f}{q3 - q1:>9.3f}{nbytes:>8.2f}{elems * nbytes / q2 / 1e6:>9.0f}")
lines.append(f"(b)/(a) = {med['b'][0] / med['a'][0]:.3f}   (36 B / 28 B = 1.286 if both stream at the same rate)")
lines.append(f"(b)/(c) = {med['b'][0] / med['c'][0]:.3f}   ((c) - (b) = {med['c'][0] - med['b'][0]:.3f} ms against an IQR of "
             f"{max(med['b'][1], med['c'][1]):.3f} ms; 36 B / 40 B = 0.900 from bytes alone, plus one launch)")
for u, g in (("d", "e"), ("f", "g")):
    if u in med and g in med:
        lines.append(f"({g})/({u}) = {med[g][0] / med[u][0]:.4f}   (guarded - unguarded = {med[g][0] - med[u][0]:+.4f} ms against an IQR of "
                     f"{max(med[u][1], med[g][1]):.4f} ms)")
lines.append(f"library: {os.environ.get('KAI0_HIP_LIB', 'in-tree')}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
