"""The Gemma MLP's weight gradients alone, as they launch today (TN: both operands [contraction][cols], the ring loop) against the
same products with both operands K-contiguous (NT: the 256 x 256 quadrant tile kernel; 512 / 1024 tiles are below the persistent rule): ms per launch and TFLOP/s on random data, graph-replayed,
both arms in ONE process, alternating.  The NT arm's operands are the transposes of the TN arm's, so both compute the same matrix.
usage: python tools/probes/mlp_wgrad_nt.py [rows]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from kai0_amd import ops  # noqa: E402

BF16 = torch.bfloat16
dev = torch.device("cuda:0")
REPS = 4
ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 30976  # the prefix's rows at B = 32
D, F = 2048, 16384


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def timeit(g):
    ts = []
    for _ in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return min(ts) / REPS


def case(name, n, k, pieces=1):
    """dW [pieces * n, k] = dy^T @ inp over ROWS.  TN: `pieces` launches of dy_i [ROWS, n], inp [ROWS, k] (today's wgrad()).
    NT: ONE launch of dyT [pieces * n, ROWS] (the pieces stacked along M), inpT [k, ROWS]."""
    gen = torch.Generator(device=dev).manual_seed(n + k + pieces)
    dys = [(torch.randn(ROWS, n, device=dev, generator=gen) * 0.05).to(BF16) for _ in range(pieces)]
    inp = (torch.randn(ROWS, k, device=dev, generator=gen) * 0.05).to(BF16)
    dyT = torch.cat([d.t().contiguous() for d in dys], 0)
    inpT = inp.t().contiguous()
    dw_tn = torch.empty(pieces * n, k, device=dev, dtype=BF16)
    dw_nt = torch.empty(pieces * n, k, device=dev, dtype=BF16)
    split = ops.pick_split_k_wgrad(n, k, ROWS)

    def tn():
        for i, dy in enumerate(dys):
            ops.gemm(dy, inp, dw_tn[i * n:(i + 1) * n], M=n, N=k, K=ROWS, a_kc=False, b_kc=False, lda=n, ldb=k, ldc=k, split_k=split, nt_out=True)

    def nt():
        ops.gemm(dyT, inpT, dw_nt, M=pieces * n, N=k, K=ROWS, lda=ROWS, ldb=ROWS, ldc=k, split_k=1, nt_out=True)

    plan_tn = ops.gemm_plan(dys[0], inp, dw_tn, M=n, N=k, K=ROWS, a_kc=False, b_kc=False, lda=n, ldb=k, ldc=k, split_k=split, nt_out=True)
    plan_nt = ops.gemm_plan(dyT, inpT, dw_nt, M=pieces * n, N=k, K=ROWS, lda=ROWS, ldb=ROWS, ldc=k, split_k=1, nt_out=True)
    g_tn, g_nt = graph_of(tn), graph_of(nt)
    t_tn, t_nt = [], []
    for _ in range(3):  # alternating passes
        t_tn.append(timeit(g_tn))
        t_nt.append(timeit(g_nt))
    same = bool(torch.equal(dw_tn, dw_nt))
    rel = float((dw_tn.float() - dw_nt.float()).norm() / dw_nt.float().norm())
    fl = 2.0 * pieces * n * k * ROWS
    a, b = min(t_tn), min(t_nt)
    print(f"{name:28s} {pieces * n} x {k} x {ROWS}: TN ({pieces} launch, {plan_tn['loop']}, split {split}) {a:6.3f} ms {fl / a * 1e-9:5.0f} TFLOP/s"
          f"   NT (1 launch, {plan_nt['loop']}) {b:6.3f} ms {fl / b * 1e-9:5.0f} TFLOP/s   NT/TN time {b / a:.3f}   bit-equal {same}  rel-L2 {rel:.1e}", flush=True)
    print(f"    passes TN {['%.3f' % t for t in t_tn]}  NT {['%.3f' % t for t in t_nt]}", flush=True)


case("down wgrad", D, F)
case("gate (or up) wgrad", F, D)
case("gate | up wgrad, one launch", F, D, pieces=2)
