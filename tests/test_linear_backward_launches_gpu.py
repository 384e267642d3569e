"""The launch sequence of every autograd shim that computes a Linear's gradients: ops.linear, ops.linear_multi (stacked, stacked over
back-to-back buffers, and one weight at a time), ops.geglu_mlp, ops.gelu_mlp, lora.lora_linear and lora.lora_geglu_mlp.

One forward and one backward per case run with three recorders in place (ops.gemm; lora.gemm, which lora.py binds at import;
_lib.call) and with every parameter publishing a gradient destination (`_kai0_grad_out`) and an arrival callback (`_kai0_grad_done`) as
the sharded trainer does.  The record is the ordered list of

  ("gemm", a_kc, b_kc, M, N, K, lda, ldb, ldc, split_k, accumulate, nt_out, act, ct is not None, ct2 is not None)
  ("call", entry point)          every _lib.call but kai0_gemm_bf16 (the "gemm" events) and kai0_gemm_plan (launches nothing)
  ("done", parameter name)       the trainer's bucket bookkeeping sees this order

and is compared with a table written out here by hand from the shims' code: which weight goes through its transpose and the
K-contiguous form (rows >= 4096), which NN launch takes ops.pick_split_k and which stays unsplit, which weight gradient is stored
non-temporally, which operands are read with a padded row stride, and when the trainer is told.  Only the split factors come from
ops.pick_split_k / ops.pick_split_k_wgrad.  The shapes are the smallest that reach every branch: 4088 and 4096 rows around the
threshold, every dimension a multiple of 8.  A refactor of the backward passes leaves every table as it is."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda:0"
T, F = True, False


@pytest.fixture(scope="module")
def mods():
    from kai0_amd import _lib, lora, ops

    return ops, lora, _lib


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16).to(DEV)


def G(a_kc, b_kc, M, N, K, lda, ldb, ldc, split_k=1, accumulate=False, nt_out=False, act=0, ct=False, ct2=False):
    return ("gemm", a_kc, b_kc, M, N, K, lda, ldb, ldc, split_k, accumulate, nt_out, act, ct, ct2)


def call(name):
    return ("call", name)


def done(*names):
    return [("done", n) for n in names]


TRANSPOSE = call("kai0_transpose_bf16")
COLSUM = call("kai0_colsum_partials_bf16")
REDUCE = call("kai0_reduce_partials_batch")  # the queued final sums of the bias gradients: one launch when the backward pass ends
LORA_DOWN, LORA_WGRAD = call("kai0_lora_down"), call("kai0_lora_wgrad")


def record(mods, monkeypatch, params, run, dsts=None):
    """The events of `run()`.  `params` {name: leaf tensor}: each gets a NaN-filled gradient destination (`dsts[name]` if given) and
    must have reported its arrival, with a finite gradient in that destination, by the time `run` returns."""
    ops, lora, _lib = mods
    events = []
    real_gemm, real_call = ops.gemm, _lib.call

    def gemm(A, B, out, **kw):
        events.append(("gemm", kw.get("a_kc", True), kw.get("b_kc", True), kw["M"], kw["N"], kw["K"], kw["lda"], kw["ldb"], kw["ldc"],
                       kw.get("split_k", 1), kw.get("accumulate", False), kw.get("nt_out", False), kw.get("act", 0),
                       kw.get("ct") is not None, kw.get("ct2") is not None))  # fmt: skip
        return real_gemm(A, B, out, **kw)

    def lib_call(name, *args):
        if name not in ("kai0_gemm_bf16", "kai0_gemm_plan"):
            events.append(("call", name))
        return real_call(name, *args)

    for name, p in params.items():
        p.requires_grad_(True)
        p._kai0_grad_out = dsts[name] if dsts else torch.empty_like(p)
        p._kai0_grad_out.fill_(float("nan"))
        p._kai0_grad_done = lambda name=name: events.append(("done", name))
    ops.reset_backward_state()
    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(lora, "gemm", gemm)
    monkeypatch.setattr(_lib, "call", lib_call)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(ops, "gemm", real_gemm)
        monkeypatch.setattr(lora, "gemm", real_gemm)
        monkeypatch.setattr(_lib, "call", real_call)
    for name, p in params.items():
        assert p.grad is None and torch.isfinite(p._kai0_grad_out).all(), f"{name}: no gradient in its destination"
    return events


def check(events, expected):
    for i, (e, x) in enumerate(zip(events, expected)):
        assert e == x, f"event {i}: recorded {e}, expected {x}\nrecorded: {events}"
    assert len(events) == len(expected), f"recorded {events[len(expected):]} past the table / table not reached: {expected[len(events):]}"


# ------------------------------------------------------------------------------------------------------ ops.linear
@pytest.mark.parametrize("M", [4088, 4096])
def test_linear(mods, monkeypatch, M):
    """bias, residual, GELU.  Below 4096 rows: the NN dgrad with pick_split_k; from 4096: W transposed once, the NT dgrad, unsplit."""
    ops = mods[0]
    K, N = 200, 264
    x, res, dy = rnd(M, K, seed=1).requires_grad_(True), rnd(M, N, seed=2).requires_grad_(True), rnd(M, N, seed=3)
    p = {"w": rnd(N, K, seed=4, scale=0.08), "bias": rnd(N, seed=5)}
    ev = record(mods, monkeypatch, p, lambda: ops.linear(x, p["w"], p["bias"], res, 1).backward(dy))
    dgrad = ([TRANSPOSE, G(T, T, M, K, N, N, N, K)] if M >= 4096 else
             [G(T, F, M, K, N, N, K, K, split_k=ops.pick_split_k(M, K, N))])  # fmt: skip
    check(ev, [G(T, T, M, N, K, K, K, N, split_k=ops.pick_split_k(M, N, K), act=1),
               call("kai0_gelu_bwd"),
               *dgrad,
               G(F, F, N, K, M, N, K, K, split_k=ops.pick_split_k_wgrad(N, K, M), nt_out=True),
               COLSUM, *done("bias", "w"), REDUCE])  # fmt: skip
    assert torch.isfinite(x.grad).all() and torch.equal(res.grad, dy)


# ------------------------------------------------------------------------------------------------ ops.linear_multi
WIDTHS = (136, 72, 72)
NT_ = sum(WIDTHS)  # 280
KM = 136


def multi_inputs(M, flat):
    x = rnd(M, KM, seed=1).requires_grad_(True)
    douts = [rnd(M, n, seed=20 + i) for i, n in enumerate(WIDTHS)]
    p, dsts = {}, None
    if flat:  # q | k | v weights back to back in one buffer, as in a trainer's flat parameter buffer, and their gradients likewise
        wflat, gflat = rnd(NT_, KM, seed=2, scale=0.1), torch.empty((NT_, KM), dtype=BF16, device=DEV)
        r, dsts = 0, {}
        for i, n in enumerate(WIDTHS):
            p[f"w{i}"], dsts[f"w{i}"] = wflat[r : r + n], gflat[r : r + n]
            r += n
    else:
        for i, n in enumerate(WIDTHS):
            p[f"w{i}"] = rnd(n, KM, seed=2 + i, scale=0.1)
    for i, n in enumerate(WIDTHS):
        p[f"b{i}"] = rnd(n, seed=10 + i)
        if dsts is not None:
            dsts[f"b{i}"] = torch.empty(n, dtype=BF16, device=DEV)
    return x, p, dsts, douts


def multi_forward(ops, M):
    return G(T, T, M, NT_, KM, KM, KM, WIDTHS[0], split_k=ops.pick_split_k(M, NT_, KM))


@pytest.mark.parametrize("M,flat", [(4088, False), (4096, False), (4096, True)])
def test_linear_multi_stacked(mods, monkeypatch, M, flat):
    """One dgrad over the stacked weight (NN and UNSPLIT below 4096 rows, NT from 4096) and one wgrad over the stacked dY WITHOUT the
    non-temporal store: into a temporary that is copied out, or (flat) straight into the back-to-back gradient destinations."""
    ops = mods[0]
    x, p, dsts, douts = multi_inputs(M, flat)

    def run():
        outs = ops.linear_multi(x, [p[f"w{i}"] for i in range(3)], [p[f"b{i}"] for i in range(3)])
        torch.autograd.backward(list(outs), douts)

    ev = record(mods, monkeypatch, p, run, dsts)
    dgrad = [TRANSPOSE, G(T, T, M, KM, NT_, NT_, NT_, KM)] if M >= 4096 else [G(T, F, M, KM, NT_, NT_, KM, KM)]
    check(ev, [multi_forward(ops, M),
               *dgrad,
               G(F, F, NT_, KM, M, NT_, KM, KM, split_k=ops.pick_split_k_wgrad(NT_, KM, M)),
               *done("w0", "w1", "w2"),
               COLSUM, *done("b0", "b1", "b2"), REDUCE])  # fmt: skip
    assert torch.isfinite(x.grad).all()


@pytest.mark.parametrize("M", [4088, 4096])
def test_linear_multi_one_output_unused(mods, monkeypatch, M):
    """A None among the output gradients sends the backward through one weight at a time: the dgrads accumulate into one dx (NN and
    unsplit below 4096 rows, NT from 4096), every weight gradient is a launch of its own WITH the non-temporal store, and the unused
    projection launches nothing.  Autograd hands a Function zeros for an unused output, never None, so the node's backward is called
    directly here: outside a backward pass a queued bias sum runs at once, which is why each bias has its own final sum."""
    ops = mods[0]
    x, p, _, douts = multi_inputs(M, False)
    unused = ("w2", "b2")
    used = {k: v for k, v in p.items() if k not in unused}
    for k in unused:
        p[k].requires_grad_(True)
    got = []

    def run():
        outs = ops.linear_multi(x, [p[f"w{i}"] for i in range(3)], [p[f"b{i}"] for i in range(3)])
        got.extend(ops.LinearMultiFn.backward(outs[0].grad_fn, douts[0], douts[1], None))

    ev = record(mods, monkeypatch, used, run)
    expected = [multi_forward(ops, M)]
    for i, n in enumerate(WIDTHS[:2]):
        expected += ([TRANSPOSE, G(T, T, M, KM, n, n, n, KM, accumulate=i > 0)] if M >= 4096 else
                     [G(T, F, M, KM, n, n, KM, KM, accumulate=i > 0)])  # fmt: skip
        expected += [G(F, F, n, KM, M, n, KM, KM, split_k=ops.pick_split_k_wgrad(n, KM, M), nt_out=True), *done(f"w{i}"),
                     COLSUM, REDUCE, *done(f"b{i}")]  # fmt: skip
    check(ev, expected)
    assert torch.isfinite(got[0]).all() and all(g is None for g in got[1:])


# --------------------------------------------------------------------------------------------------- ops.geglu_mlp
@pytest.mark.parametrize("M,Fd,flat", [(1600, 512, False), (4096, 512, False), (4096, 2560, False), (4096, 2560, True)])
def test_geglu_mlp(mods, monkeypatch, M, Fd, flat):
    """The three dgrads go through the transposed weight at EVERY row count.  The weight gradients are TN launches, except where the
    producers' launches take the 256 x 256 tile (4096 rows, F = 2560): those store hT and dgT | duT (ct / ct2) and the weight
    gradients read them K-contiguous — as one M = 2 F launch when the gate and up destinations lie back to back (flat)."""
    ops = mods[0]
    D = 256
    x, dout = rnd(M, D, seed=1).requires_grad_(True), rnd(M, D, seed=2)
    p, dsts = {"wd": rnd(D, Fd, seed=5, scale=0.05)}, None
    if flat:
        wflat, gflat = rnd(2 * Fd, D, seed=3, scale=0.05), torch.empty((2 * Fd, D), dtype=BF16, device=DEV)
        p.update(wg=wflat[:Fd], wu=wflat[Fd:])
        dsts = {"wg": gflat[:Fd], "wu": gflat[Fd:], "wd": torch.empty((D, Fd), dtype=BF16, device=DEV)}
    else:
        p.update(wg=rnd(Fd, D, seed=3, scale=0.05), wu=rnd(Fd, D, seed=4, scale=0.05))
    ev = record(mods, monkeypatch, p, lambda: ops.geglu_mlp(x, p["wg"], p["wu"], p["wd"]).backward(dout), dsts)
    nt = M >= 4096 and Fd == 2560
    wsplit = ops.pick_split_k_wgrad
    if nt:
        down = [TRANSPOSE, G(T, T, D, Fd, M, M, M, Fd, split_k=wsplit(D, Fd, M), nt_out=True)]
        gate_up = [TRANSPOSE] + ([G(T, T, 2 * Fd, D, M, M, M, D, split_k=wsplit(2 * Fd, D, M), nt_out=True)] if flat else
                                 [G(T, T, Fd, D, M, M, M, D, split_k=wsplit(Fd, D, M), nt_out=True)] * 2)  # fmt: skip
    else:
        down = [G(F, F, D, Fd, M, D, Fd, Fd, split_k=wsplit(D, Fd, M), nt_out=True)]
        gate_up = [G(F, F, Fd, D, M, Fd, D, D, split_k=wsplit(Fd, D, M), nt_out=True)] * 2
    check(ev, [G(T, T, M, Fd, D, D, D, Fd, act=6, ct=nt),
               G(T, T, M, D, Fd, Fd, Fd, D, split_k=ops.pick_split_k(M, D, Fd)),
               *down,
               TRANSPOSE, G(T, T, M, Fd, D, D, D, Fd, act=3, ct=nt, ct2=nt),
               *gate_up,
               TRANSPOSE, G(T, T, M, D, Fd, Fd, Fd, D),
               TRANSPOSE, G(T, T, M, D, Fd, Fd, Fd, D, accumulate=True),
               *done("wg", "wu", "wd")])  # fmt: skip
    assert torch.isfinite(x.grad).all()


# ---------------------------------------------------------------------------------------------------- ops.gelu_mlp
@pytest.mark.parametrize("M", [4088, 4096])
def test_gelu_mlp(mods, monkeypatch, M):
    """F = 136 in rows padded to ldh = 192.  The act-5 dgrad (C rows of ldh) is NN and UNSPLIT below 4096 rows, the dx dgrad (A rows
    of ldh) NN with pick_split_k; both NT from 4096.  The trainer hears of each weight gradient right after its launch."""
    ops = mods[0]
    D, Fd, ldh = 64, 136, 192
    x, res, dout = rnd(M, D, seed=1).requires_grad_(True), rnd(M, D, seed=2).requires_grad_(True), rnd(M, D, seed=3)
    p = {"w1": rnd(Fd, D, seed=4, scale=0.1), "b1": rnd(Fd, seed=5), "w2": rnd(D, Fd, seed=6, scale=0.1), "b2": rnd(D, seed=7)}
    ev = record(mods, monkeypatch, p, lambda: ops.gelu_mlp(x, p["w1"], p["b1"], p["w2"], p["b2"], res).backward(dout))
    big = M >= 4096
    check(ev, [G(T, T, M, Fd, D, D, D, ldh, act=1),
               G(T, T, M, D, Fd, ldh, Fd, D, split_k=ops.pick_split_k(M, D, Fd)),
               G(F, F, D, Fd, M, D, ldh, Fd, split_k=ops.pick_split_k_wgrad(D, Fd, M), nt_out=True), *done("w2"),
               COLSUM, *done("b2"),
               *([TRANSPOSE, G(T, T, M, Fd, D, D, D, ldh, act=5)] if big else [G(T, F, M, Fd, D, D, Fd, ldh, act=5)]),
               G(F, F, Fd, D, M, ldh, D, D, split_k=ops.pick_split_k_wgrad(Fd, D, M), nt_out=True), *done("w1"),
               COLSUM, *done("b1"),
               *([TRANSPOSE, G(T, T, M, D, Fd, ldh, Fd, D)] if big else
                 [G(T, F, M, D, Fd, ldh, D, D, split_k=ops.pick_split_k(M, D, Fd))]),
               REDUCE])  # fmt: skip
    assert torch.isfinite(x.grad).all() and torch.equal(res.grad, dout)


# ------------------------------------------------------------------------------------------------ lora.lora_linear
@pytest.mark.parametrize("M", [4088, 4096])
def test_lora_linear(mods, monkeypatch, M):
    """The base weight's dgrad and wgrad are ops.linear's launches; the adapter's products stand around them."""
    ops, lora, _ = mods
    K, N, r = 200, 264, 16
    x, dy = rnd(M, K, seed=1).requires_grad_(True), rnd(M, N, seed=2)
    p = {"w": rnd(N, K, seed=3, scale=0.08), "a": rnd(r, K, seed=4, scale=0.1), "b": rnd(N, r, seed=5, scale=0.1)}
    ev = record(mods, monkeypatch, p, lambda: lora.lora_linear(x, p["w"], lora.Adapter(p["a"], p["b"], 2.0)).backward(dy))
    dgrad = ([TRANSPOSE, G(T, T, M, K, N, N, N, K)] if M >= 4096 else
             [G(T, F, M, K, N, N, K, K, split_k=ops.pick_split_k(M, K, N))])  # fmt: skip
    check(ev, [G(T, T, M, N, K, K, K, N, split_k=ops.pick_split_k(M, N, K)),
               LORA_DOWN, G(T, T, M, N, r, r, r, N, accumulate=True),  # T = x A^T; y += s T B^T
               TRANSPOSE, LORA_DOWN,  # dT = dy B through B^T
               *dgrad,
               G(T, F, M, K, r, r, K, K, accumulate=True),  # dx += s dT A
               G(F, F, N, K, M, N, K, K, split_k=ops.pick_split_k_wgrad(N, K, M), nt_out=True),
               LORA_WGRAD, LORA_WGRAD,
               *done("w", "a", "b")])  # fmt: skip
    assert torch.isfinite(x.grad).all()


# --------------------------------------------------------------------------------------------- lora.lora_geglu_mlp
def test_lora_geglu_mlp(mods, monkeypatch):
    """dx = dg Wg + du Wu as two dgrads, the second accumulating into the first's output (NT at 4096 rows; unsplit either way)."""
    ops, lora, _ = mods
    M, D, Fd, r = 4096, 256, 512, 16
    x, dout = rnd(M, D, seed=1).requires_grad_(True), rnd(M, D, seed=2)
    p = {"wg": rnd(Fd, D, seed=3, scale=0.05), "wu": rnd(Fd, D, seed=4, scale=0.05), "wd": rnd(D, Fd, seed=5, scale=0.05),
         "ag": rnd(r, D, seed=6, scale=0.1), "bg": rnd(Fd, r, seed=7, scale=0.1), "au": rnd(r, D, seed=8, scale=0.1),
         "bu": rnd(Fd, r, seed=9, scale=0.1), "ad": rnd(r, Fd, seed=10, scale=0.1), "bd": rnd(D, r, seed=11, scale=0.1)}  # fmt: skip

    def run():
        A = lora.Adapter
        lora.lora_geglu_mlp(x, p["wg"], p["wu"], p["wd"], A(p["ag"], p["bg"]), A(p["au"], p["bu"]), A(p["ad"], p["bd"])).backward(dout)

    ev = record(mods, monkeypatch, p, run)
    wsplit = ops.pick_split_k_wgrad
    Kc = D + r
    check(ev, [G(T, T, M, Fd, D, D, D, Fd, split_k=ops.pick_split_k(M, Fd, D)),  # g
               G(T, T, M, Fd, D, D, D, Fd, split_k=ops.pick_split_k(M, Fd, D)),  # u
               LORA_DOWN,  # Tgu [M, 2 r]
               G(T, T, M, Fd, r, 2 * r, r, Fd, accumulate=True), G(T, T, M, Fd, r, 2 * r, r, Fd, accumulate=True),
               call("kai0_geglu_fwd"),
               G(T, T, M, D, Fd, Fd, Fd, D, split_k=ops.pick_split_k(M, D, Fd)),
               LORA_DOWN, G(T, T, M, D, r, r, r, D, accumulate=True),
               # backward
               G(F, F, D, Fd, M, D, Fd, Fd, split_k=wsplit(D, Fd, M), nt_out=True),  # dWd
               LORA_WGRAD,  # dBd
               TRANSPOSE, LORA_DOWN,  # dTd into [dout | dTd]
               call("kai0_transpose_strided_bf16"), call("kai0_transpose_strided_bf16"),  # [Wd^T | Ad^T]
               LORA_WGRAD,  # dAd
               G(T, T, M, Fd, Kc, Kc, Kc, Fd, act=3),
               G(F, F, Fd, D, M, Fd, D, D, split_k=wsplit(Fd, D, M), nt_out=True),  # dWg
               G(F, F, Fd, D, M, Fd, D, D, split_k=wsplit(Fd, D, M), nt_out=True),  # dWu
               LORA_WGRAD, LORA_WGRAD,  # dBg, dBu
               TRANSPOSE, LORA_DOWN, TRANSPOSE, LORA_DOWN,  # dTgu
               LORA_WGRAD,  # dAg | dAu
               TRANSPOSE, G(T, T, M, D, Fd, Fd, Fd, D),
               TRANSPOSE, G(T, T, M, D, Fd, Fd, Fd, D, accumulate=True),
               G(T, F, M, D, 2 * r, 2 * r, D, D, accumulate=True),  # dx += dTgu Agu
               *done("wg", "wu", "wd", "ag", "bg", "au", "bu", "ad", "bd")])  # fmt: skip
    assert torch.isfinite(x.grad).all()
