"""The bits the optimizer kernels write, for comparing two builds of libkai0hip.so: the four AdamW entry points and kai0_grad_accum
(with and without its sum of squares) over heads, tails, alignment fallbacks, dtype pairs and row flags, from CPU seeds, through
the C ABI (kai0_amd._lib.call) — nothing of the Python API above it is involved.  One SHA-256 per buffer (guard elements around
every view included) goes to a JSON file; run it once per library (KAI0_HIP_LIB selects it, one process each) and compare.
usage: python tools/probes/optim_bits.py --out A.json
       python tools/probes/optim_bits.py --compare A.json B.json      (exit status 1 on any difference)"""
import argparse
import hashlib
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
args = ap.parse_args()
if args.compare:
    a, b = (json.load(open(p)) for p in args.compare)
    bad = sorted(k for k in a.keys() | b.keys() if a.get(k) != b.get(k))
    for k in bad[:20]:
        print(f"DIFFERENT {k}: {a.get(k)} / {b.get(k)}")
    print(f"{len(a)} / {len(b)} cases, {sum(len(v) for v in a.values())} digests, {len(bad)} cases differ")
    sys.exit(1 if bad or not a else 0)
if not args.out:
    ap.error("--out or --compare")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from kai0_amd import _lib  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("optim_bits.py runs the kernels; there is no GPU here")
DEV, F32, BF16, GUARD = torch.device("cuda:0"), torch.float32, torch.bfloat16, 16
gen = torch.Generator().manual_seed(20)
ADAM = (1e-3, 0.9, 0.95, 1e-8, 1e-2, 1 - 0.9**3, 1 - 0.95**3)  # lr, beta1, beta2, eps, wd, bc1, bc2
ADAM_ROWS = (2.5e-5, 0.9, 0.95, 1e-8, 1e-10, 1 - 0.9**3, 1 - 0.95**3)  # lr * wd rounds away
coef = torch.tensor([0.37], device=DEV)
digests = {}


def call(name, *a):
    _lib.call(name, *a, torch.cuda.current_stream().cuda_stream)


class Buf:
    """`values` as a view `off` elements past a 16-byte boundary, GUARD elements of 7.0 on both sides."""

    def __init__(self, values, dtype, off):
        n = values.numel()
        self.whole = torch.full((GUARD + off + n + GUARD,), 7.0, dtype=dtype, device=DEV)
        self.t = self.whole[GUARD + off : GUARD + off + n]
        self.t.copy_(values.reshape(-1).to(DEV))
        assert self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        self.p = self.t.data_ptr()

    def sha(self):
        return hashlib.sha256(self.whole.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def randn(*shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def record(case, **bufs):
    torch.cuda.synchronize()
    digests[case] = {k: b.sha() for k, b in bufs.items()}


LAYOUTS = {"aligned": (0, 0), "one_in": (1, 1), "no_common_head": (1, 0)}  # offsets of the f32 / the 16-bit streams
for n in (1, 3, 5, 255, 1027, 4099, 2**20 + 3):
    master, m, v, g = randn(n, scale=0.02), randn(n, scale=1e-2), randn(n, scale=1e-2).abs(), randn(n).to(BF16)
    ema = master + randn(n, scale=1e-3)
    for layout, (off32, off16) in LAYOUTS.items():
        for g_f32 in ((0,) if n > 2**20 else (0, 1)):
            for p_f32 in (0, 1):
                gdt, goff = (F32, off32) if g_f32 else (BF16, off16)
                pdt, poff = (F32, off32) if p_f32 else (BF16, off16)
                for clip in (None, coef.data_ptr()):
                    for with_ema in (0, 1):
                        st = [Buf(t, F32, off32) for t in (master, m, v)]
                        e, grad, param = Buf(ema, F32, off32), Buf(g, gdt, goff), Buf(torch.full((n,), float("nan")), pdt, poff)
                        tail = (g_f32, param.p, p_f32, n, *ADAM)
                        if with_ema:
                            call("kai0_adamw_ema", st[0].p, st[1].p, st[2].p, e.p, grad.p, *tail, 0.99, clip)
                        else:
                            call("kai0_adamw", st[0].p, st[1].p, st[2].p, grad.p, *tail, clip)
                        record(f"adamw{'_ema' * with_ema} n={n} {layout} g_f32={g_f32} p_f32={p_f32} clip={clip is not None}",
                               master=st[0], m=st[1], v=st[2], ema=e, param=param, grad=grad)

for rows, rl in ((37, 8), (19, 12), (19, 6), (5, 2056)):
    n = rows * rl
    live = torch.tensor([i % 3 != 1 for i in range(rows)])
    flagged = torch.tensor([i % 6 == 1 for i in range(rows)])  # no gradient, but moments from earlier steps: updated all the same
    master, g = randn(rows, rl, scale=0.02), randn(rows, rl).to(BF16)
    m, v = randn(rows, rl, scale=1e-2), randn(rows, rl, scale=1e-2).abs()
    m[~(live | flagged)] = 0
    v[~(live | flagged)] = 0
    ema = master.clone()
    ema[live | flagged] += 1e-3
    g[~live] = 0
    g[~live, ::2] = -0.0
    for off in (0, 1):
        for g_f32 in (0, 1):
            for p_f32 in (0, 1):
                for clip in (None, coef.data_ptr()):
                    for with_ema in (0, 1):
                        st = [Buf(t, F32, off) for t in (master, m, v)]
                        e, grad = Buf(ema, F32, off), Buf(g, F32 if g_f32 else BF16, off)
                        param = Buf(master, F32 if p_f32 else BF16, off)
                        active = Buf(flagged.to(torch.uint8), torch.uint8, 0)
                        tail = (g_f32, param.p, p_f32, rows, rl, active.p, *ADAM_ROWS)
                        if with_ema:
                            call("kai0_adamw_rows_ema", st[0].p, st[1].p, st[2].p, e.p, grad.p, *tail, 0.99, clip)
                        else:
                            call("kai0_adamw_rows", st[0].p, st[1].p, st[2].p, grad.p, *tail, clip)
                        record(f"adamw_rows{'_ema' * with_ema} {rows}x{rl} off={off} g_f32={g_f32} p_f32={p_f32} clip={clip is not None}",
                               master=st[0], m=st[1], v=st[2], ema=e, param=param, active=active)

scratch = torch.zeros(4096, device=DEV)
for n in (1, 3, 5, 255, 1027, 4099, 2**20 + 3):
    acc0, g = randn(n), randn(n).to(BF16)
    for layout, (aoff, off16) in LAYOUTS.items():
        for g_f32 in ((0,) if n > 2**20 else (0, 1)):
            for first in (0, 1):
                for sumsq in (0, 1):
                    acc, grad = Buf(acc0, F32, aoff), Buf(g, F32 if g_f32 else BF16, aoff if g_f32 else off16)
                    out = Buf(torch.tensor([0.25]), F32, 0)
                    call("kai0_grad_accum", acc.p, grad.p, g_f32, n, first, out.p if sumsq else None, scratch.data_ptr() if sumsq else None)
                    record(f"grad_accum n={n} {layout} g_f32={g_f32} first={first} sumsq={sumsq}", acc=acc, sumsq=out)

json.dump(digests, open(args.out, "w"), indent=0, sort_keys=True)
print(f"{len(digests)} cases, {sum(len(v) for v in digests.values())} digests -> {args.out}; library {os.environ.get('KAI0_HIP_LIB', _lib.LIB_PATH)}")
