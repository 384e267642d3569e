"""Skipping optimizer steps whose gradient norm is not finite, on the MI355X: kai0_clip_coef_guard, the negative clip coefficient
(KAI0_COEF_SKIP) in all four AdamW entry points, the Trainer on the tiny model across a poisoned step, FusedAdamW.  The kernels are
called through the C ABI (kai0_amd._lib.call) as in tests/test_streaming_kernels_gpu.py.

Everything is bit for bit: a skipped launch must leave every byte alone (buffers and the 16 elements on both sides of them are
pre-filled with random bits and compared as integers), and a launch that is not skipped must be what it was.

The normal path against tests/streaming_refs.adamw, bit for bit.  `adamw(..., dt=float32)` is the update written as single f32
operations in the kernel's order (no multiply is fused into an add on either side), with two exceptions: it divides by bc1 and by
sqrt(bc2) where the kernel multiplies by 1.0f / bc1 and rsqrtf(bc2).  The bias corrections are arguments of the entry points, so the
launches here pass bc1 = 0.5 and bc2 = 0.25 (t = 1 with beta1 = 0.5, beta2 = 0.75): both reciprocals are powers of two, multiplying
and dividing by them is the same exact operation, and the f32 evaluation is the kernel's arithmetic operation by operation.  With
general bias corrections the two differ in the last bit of some elements by construction; that case stays with the float64 bound
of tests/test_streaming_kernels_gpu.py.
The reference is evaluated on the CPU, where torch's f32 multiply, add, subtract and divide are the IEEE operations — but not its
square root: it goes through a vector math library that is good to an ulp without being correctly rounded (18 of this test's 3079
roots differ from numpy's, which are the IEEE ones, on one host and other elements on another; the GPU backend's differ likewise).
The kernel's sqrtf is the correctly rounded one, so `ieee_sqrt` stands in for `torch.sqrt` while streaming_refs.adamw runs."""

import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import streaming_refs as R  # noqa: E402
from streaming_refs import BF16, F32  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8 = torch.uint8
INF, NAN = float("inf"), float("nan")
GUARD = 16
EMA_DECAY = 0.99
# lr, beta1, beta2, eps, wd, bc1, bc2 (module docstring: bc1, bc2 with power-of-two reciprocals); the row forms need 1 - lr * wd == 1
HYPER = {"dense": (1e-3, 0.9, 0.95, 1e-8, 1e-2, 0.5, 0.25), "rows": (2.5e-5, 0.9, 0.95, 1e-8, 1e-10, 0.5, 0.25)}
N = 3079  # 769 vectors of four (four blocks of 256 lanes) + a scalar tail of 3; started 3 elements in: a scalar head of 1, a tail of 2
DENSE_SHAPES = [(N, 0), (N, 3), (3, 0)]  # (elements, elements past a 16-byte boundary at which every stream starts)
ROWS_SHAPES = [(5, 24), (5, 23)]  # vector rows, scalar rows; rows 1 and 3 idle
IDLE = (1, 3)


def call(name, *args):
    from kai0_amd import _lib

    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


class Buf:
    """`n` elements `off` past a 16-byte boundary inside an allocation of random bits (GUARD elements on both sides)."""

    def __init__(self, n, dtype, off, gen, init=None):
        itype = {F32: torch.int32, BF16: torch.int16, U8: torch.uint8}[dtype]
        info = torch.iinfo(itype)
        raw = torch.randint(info.min, info.max + 1, (GUARD + off + n + GUARD,), generator=gen).to(itype).to(DEV)
        self.raw, self.lo, self.n = raw, GUARD + off, n
        self.t = raw.view(dtype)[self.lo : self.lo + n]
        assert self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        if init is not None:
            self.t.copy_(init.to(DEV))
        self.before = raw.clone()

    @property
    def p(self):
        return self.t.data_ptr()

    def untouched(self):
        return torch.equal(self.raw, self.before)

    def bands_untouched(self):
        return torch.equal(self.raw[: self.lo], self.before[: self.lo]) and torch.equal(self.raw[self.lo + self.n :], self.before[self.lo + self.n :])


# ================================================================================================ 1. kai0_clip_coef_guard
def test_clip_coef_guard_is_clip_coef_on_finite_sums_and_the_sentinel_otherwise():
    from kai0_amd.optim import COEF_SKIP

    sumsq = torch.zeros(1, device=DEV)
    skipped = torch.zeros(1, dtype=torch.int32, device=DEV)

    def both(s, max_norm):
        out = []
        for name, tail in (("kai0_clip_coef", ()), ("kai0_clip_coef_guard", (skipped.data_ptr(),))):
            coef, norm = torch.full((1,), -7.0, device=DEV), torch.full((1,), -7.0, device=DEV)
            sumsq.fill_(s)
            call(name, sumsq.data_ptr(), max_norm, coef.data_ptr(), norm.data_ptr(), *tail)
            torch.cuda.synchronize()
            out.append((coef, norm))
        return out

    for s in (0.0, 1e-30, 0.25, 1.0, 4.0, 1e30):
        for max_norm in (1.0, 0.37):
            (c0, n0), (c1, n1) = both(s, max_norm)
            assert torch.equal(bits(c0), bits(c1)) and torch.equal(bits(n0), bits(n1)), (s, max_norm, float(c0), float(c1))
            assert 0.0 <= float(c1) <= 1.0
        (_, n0), (c1, n1) = both(s, 0.0)  # max_norm <= 0: no clipping
        assert float(c1) == 1.0 and torch.equal(bits(n0), bits(n1)), s
        assert float(both(s, -1.0)[1][0]) == 1.0
    assert int(skipped) == 0  # none of the finite launches counted
    count = 0
    for s in (INF, NAN, -1.0, INF):  # (a negative sum has a NaN root)
        for max_norm in (1.0, 0.0):
            (c0, _), (c1, n1) = both(s, max_norm)
            count += 1
            assert float(c1) == COEF_SKIP == -1.0 and not bool(torch.isfinite(n1)) and int(skipped) == count, (s, max_norm)
            assert float(c0) >= 0.0 or float(c0) != float(c0)  # the unguarded entry never writes the sentinel
        (_, _), (c1, _) = both(4.0, 1.0)  # a finite launch in between leaves the counter alone
        assert 0.49 < float(c1) < 0.5 and int(skipped) == count  # 1 / (2 + 1e-6)
    from kai0_amd import _lib

    for args in ((None, 1.0, sumsq.data_ptr(), sumsq.data_ptr(), skipped.data_ptr()), (sumsq.data_ptr(), 1.0, sumsq.data_ptr(), sumsq.data_ptr(), None)):
        with pytest.raises(_lib.Kai0HipError, match="null buffer"):
            call("kai0_clip_coef_guard", *args)


# ================================================================================================ 2. the AdamW forms
_BASE = {}


def _base():
    """CPU inputs of length N, made once and never written to.  Gradient values are bf16 numbers: one reference serves both dtypes."""
    if not _BASE:
        _BASE.update(master=R.randn(N, seed=1, scale=0.02).float(), m=R.randn(N, dtype=F32, seed=2, scale=1e-2),
                     v=R.randn(N, dtype=F32, seed=3, scale=1e-2).abs(), grad=R.randn(N, seed=4).float())  # fmt: skip
        _BASE["ema"] = _BASE["master"] + R.randn(N, dtype=F32, seed=5, scale=1e-3)
    return _BASE


_CASES = {}


def ieee_sqrt(t):
    """The correctly rounded square root of a CPU tensor (module docstring)."""
    import numpy as np

    return torch.from_numpy(np.sqrt(t.numpy()))


def _adamw_f32(*args):
    """streaming_refs.adamw in f32 with the IEEE square root -> {master, m, v}."""
    plain = torch.sqrt
    torch.sqrt = ieee_sqrt
    try:
        ref = R.adamw(*args, F32)
    finally:
        torch.sqrt = plain
    return {k: ref[k].value for k in ("master", "m", "v")}


def _case(kind, shape):
    """Inputs (CPU, f32 values) of one shape and their f32 references per clip coefficient (0.5, None), computed once."""
    key = (kind, shape)
    if key in _CASES:
        return _CASES[key]
    b = _base()
    if kind == "dense":
        n = shape[0]
        c = {k: t[:n].clone() for k, t in b.items()}
        c["active"] = None
    else:
        rows, rl = shape
        n = rows * rl
        c = {k: t[:n].clone().view(rows, rl) for k, t in b.items()}
        for r in IDLE:  # a zero gradient (-0.0 included), zero moments, ema == master, flag clear: a fixed point the kernel skips
            c["grad"][r] = 0.0
            c["grad"][r, ::2] = -0.0
            c["m"][r] = 0.0
            c["v"][r] = 0.0
            c["ema"][r] = c["master"][r]
        c = {k: t.reshape(-1) for k, t in c.items()}
        c["active"] = torch.zeros(rows, dtype=U8)
        c["active_after"] = torch.tensor([0 if r in IDLE else 1 for r in range(rows)], dtype=U8)
    c["n"] = n
    omd = 1.0 - R.f32c(EMA_DECAY)
    c["ref"] = {}
    for coef in (0.5, None):
        out = _adamw_f32(c["master"], c["m"], c["v"], c["grad"], torch.tensor([1.0 if coef is None else coef]), *HYPER[kind])
        assert all(t.dtype == F32 for t in out.values())
        out["ema"] = c["ema"] + omd * (out["master"] - c["ema"])  # ema_element, operation by operation
        c["ref"][coef] = out
    _CASES[key] = c
    return c


def _launch(form, g_f32, p_f32, shape, bufs, hyper, coef_ptr):
    st = [bufs[k].p for k in ("master", "m", "v")]
    ema = [bufs["ema"].p] if form.endswith("ema") else []
    decay = [EMA_DECAY] if form.endswith("ema") else []
    if form.startswith("rows"):
        size = [shape[0], shape[1], bufs["active"].p]
    else:
        size = [shape[0]]
    name = {"dense": "kai0_adamw", "ema": "kai0_adamw_ema", "rows": "kai0_adamw_rows", "rows_ema": "kai0_adamw_rows_ema"}[form]
    call(name, *st, *ema, bufs["grad"].p, g_f32, bufs["param"].p, p_f32, *size, *hyper, *decay, coef_ptr)
    torch.cuda.synchronize()


@pytest.mark.parametrize("g_f32,p_f32", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("form", ["dense", "rows", "ema", "rows_ema"])
def test_adamw_forms_honour_the_sentinel_and_are_unchanged_otherwise(form, g_f32, p_f32):
    """Per form and (gradient, model copy) dtype pair, at the smallest shapes that reach each code path (DENSE_SHAPES / ROWS_SHAPES):
    coef = -1 with an all-NaN and an all-inf gradient over buffers of random bits (model copy and row flags included): every byte
    as before; coef = 0.5 and coef = nullptr on real values: master, moments and EMA equal the f32 reference bit for bit, the model
    copy is the rounded master, the row flags are set for the rows with a gradient, nothing outside the buffers is written."""
    kind = "rows" if form.startswith("rows") else "dense"
    gdt, pdt = (F32 if g_f32 else BF16), (F32 if p_f32 else BF16)
    gen = torch.Generator().manual_seed(17)
    skip = torch.tensor([-1.0], device=DEV)
    half = torch.tensor([0.5], device=DEV)
    for shape in DENSE_SHAPES if kind == "dense" else ROWS_SHAPES:
        n, off = (shape[0], shape[1]) if kind == "dense" else (shape[0] * shape[1], 0)
        what = f"{form} g_f32={g_f32} p_f32={p_f32} shape={shape}"
        for poison in (NAN, INF):
            bufs = {k: Buf(n, F32, off, gen) for k in ("master", "m", "v", "ema")}
            bufs["grad"] = Buf(n, gdt, off, gen, init=torch.full((n,), poison))
            bufs["param"] = Buf(n, pdt, off, gen)
            if kind == "rows":
                bufs["active"] = Buf(shape[0], U8, 0, gen)
            _launch(form, g_f32, p_f32, shape, bufs, HYPER[kind], skip.data_ptr())
            for k, bf in bufs.items():
                assert bf.untouched(), f"{what} poison={poison}: a skipped launch changed `{k}`"
        c = _case(kind, shape if kind == "rows" else (shape[0],))
        for coef in (0.5, None):
            bufs = {k: Buf(n, F32, off, gen, init=c[k]) for k in ("master", "m", "v", "ema")}
            bufs["grad"] = Buf(n, gdt, off, gen, init=c["grad"])
            bufs["param"] = Buf(n, pdt, off, gen, init=c["master"])
            if kind == "rows":
                bufs["active"] = Buf(shape[0], U8, 0, gen, init=c["active"])
            _launch(form, g_f32, p_f32, shape, bufs, HYPER[kind], None if coef is None else half.data_ptr())
            ref = c["ref"][coef]
            for k in ("master", "m", "v") + (("ema",) if form.endswith("ema") else ()):
                got = bufs[k].t.cpu()
                same = bits(got) == bits(ref[k])
                assert bool(same.all()), (f"{what} coef={coef}: `{k}` differs from streaming_refs.adamw (f32) in {int((~same).sum())} of {n} "
                                          f"elements, first at {int((~same).nonzero()[0])}: {float(got[~same][0])!r} vs {float(ref[k][~same][0])!r}")
            assert not torch.equal(bufs["master"].t.cpu(), c["master"]), what  # (the update is not a no-op)
            assert torch.equal(bits(bufs["param"].t), bits(bufs["master"].t.to(pdt))), f"{what} coef={coef}: model copy"
            if not form.endswith("ema"):
                assert bufs["ema"].untouched(), what
            if kind == "rows":
                assert torch.equal(bufs["active"].t.cpu(), c["active_after"]), f"{what} coef={coef}: row flags"
            assert bufs["grad"].untouched() and all(bf.bands_untouched() for bf in bufs.values()), f"{what} coef={coef}: wrote outside"


# ================================================================================================ 3. Trainer, tiny model
def _trainer(seed, micro_batch):
    from tiny import build_pair

    from kai0_amd.train import Trainer

    model, _, _, ocfg = build_pair(torch.device(DEV), seed=seed, std=0.08)
    model.train()
    tr = Trainer(model, world_size=1, rank=0, peak_lr=2e-3, warmup_steps=2, decay_steps=10, end_lr=2e-4, clip_norm=1.0,
                 bucket_bytes=1 << 16, ema_decay=0.99, micro_batch=micro_batch, skip_nonfinite=True)  # fmt: skip
    # the tiny embedding table has 304 rows: let it take the row-sparse form the real one (257152 rows) takes, so that there ARE flags
    tr.engine._SPARSE_MIN_ROWS = 256
    return tr, ocfg


def _batch(ocfg, seed, poison=False):
    from tiny import obs_to

    from oracle.pi0_oracle import synthetic_batch

    obs, actions, noise, time = synthetic_batch(ocfg, 2, seed=seed)
    if poison:
        actions[0, 0, 0] = NAN
    return obs_to(obs, torch.device(DEV)), actions.to(DEV), noise.to(DEV), time.to(DEV)


def _state(tr):
    """Parameters, masters, moments, EMA and the embedding's row flags."""
    tr.params_ready()
    out = [p.detach().clone() for p in tr.model.parameters()]
    flags = []
    for b in tr.engine.buckets:
        out += [b.master.clone(), b.exp_avg.clone(), b.exp_avg_sq.clone(), b.ema.clone()]
        flags += [seg[3].clone() for seg in getattr(b, "_sparse_segs", None) or []]
    torch.cuda.synchronize()
    return out, flags


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("micro_batch", [None, 1])
def test_trainer_skips_the_poisoned_step_and_carries_nothing_of_it_into_the_next(tmp_path, micro_batch):
    """Steps [good, one NaN in `actions`, good] with the EMA on, once as two micro-batches (the first one poisoned).  The state after
    the poisoned step is the state before it; the third step equals, bit for bit, the step of a fresh trainer that loaded the
    checkpoint written after the first step, had its step counters advanced by one and ran the same batch — a gradient buffer, an
    accumulator, a GEMM workspace or a split-K partial that carried the NaN over would show here."""
    tr, ocfg = _trainer(3, micro_batch)
    assert tr.skip_nonfinite and tr.micro_batch == micro_batch
    l1 = tr.train_step(*_batch(ocfg, 100))
    after1, flags1 = _state(tr)
    assert flags1 and 0 < sum(int(f.sum()) for f in flags1) < sum(f.numel() for f in flags1)
    assert tr.skipped_total() == 0 and bool(torch.isfinite(tr.last_grad_norm))
    ckpt = tr.save_checkpoint(str(tmp_path / "ck"))
    assert torch.load(os.path.join(ckpt, "metadata.pt"), weights_only=True)["skipped_total"] == 0
    l2 = tr.train_step(*_batch(ocfg, 101, poison=True))
    after2, flags2 = _state(tr)
    assert float(l2) != float(l2) and not bool(torch.isfinite(tr.last_grad_norm))
    assert _same(after2, after1) and _same(flags2, flags1)
    assert tr.skipped_total() == 1 and tr.global_step == 2 and tr.engine.step_count == 2
    l3 = tr.train_step(*_batch(ocfg, 102))
    after3, flags3 = _state(tr)
    n3 = tr.last_grad_norm.clone()
    assert tr.skipped_total() == 1 and all(bool(torch.isfinite(t.float()).all()) for t in after3)
    assert not _same(after3[-4:], after2[-4:])

    fresh, _ = _trainer(5, micro_batch)  # other initial weights: everything comes from the checkpoint
    assert fresh.load_checkpoint(str(tmp_path / "ck")) == 1 and fresh.engine.step_count == 1
    fresh.global_step += 1  # the skipped step consumed a schedule tick and a bias-correction step
    fresh.engine.step_count += 1
    f3 = fresh.train_step(*_batch(ocfg, 102))
    want3, wflags3 = _state(fresh)
    assert torch.equal(f3, l3) and torch.equal(fresh.last_grad_norm, n3) and float(l1) == float(l1)
    for i, (a, b) in enumerate(zip(after3, want3)):
        assert torch.equal(bits(a), bits(b)), f"tensor {i} of the state differs after the step that follows the skipped one"
    assert _same(flags3, wflags3)


# ================================================================================================ 4. FusedAdamW
@pytest.mark.parametrize("max_grad_norm", [1.0, None])
def test_fused_adamw_skips_a_poisoned_step(max_grad_norm):
    from kai0_amd.optim import FusedAdamW

    g = torch.Generator(device=DEV).manual_seed(1)
    params = [(torch.randn(100, 33, device=DEV, generator=g) * 0.02).to(BF16).requires_grad_(True),
              (torch.randn(513, device=DEV, generator=g) * 0.02).requires_grad_(True)]  # fmt: skip
    opt = FusedAdamW(params, lr=1e-2, weight_decay=1e-2, max_grad_norm=max_grad_norm, ema_decay=0.9, skip_nonfinite=True)
    assert opt.skipped_steps.dtype == torch.int32 and int(opt.skipped_steps) == 0

    def state():
        torch.cuda.synchronize()
        return [p.detach().clone() for p in params] + [t.clone() for p in params for t in opt.state[p].values()]

    states = []
    for step, poison in enumerate((None, INF, None)):
        for p in params:
            p.grad = (torch.randn(p.shape, device=DEV, generator=g) * 3).to(p.dtype)
        if poison is not None:
            params[1].grad[7] = poison
        norm = opt.step()
        assert bool(torch.isfinite(norm)) == (poison is None)
        states.append(state())
    assert _same(states[1], states[0]) and not any(torch.equal(a, b) for a, b in zip(states[2], states[1]))
    assert all(bool(torch.isfinite(t.float()).all()) for t in states[2])
    assert int(opt.skipped_steps) == 1 and opt.step_count == 3 and opt.state_dict()["skipped_steps"] == 1
    assert not hasattr(FusedAdamW(params), "skipped_steps")
