"""Gradient accumulation over micro-batches on the MI355X: the kernel `kai0_grad_accum` (bit-exact: one f32 add per element has no
freedom), its fused sum of squares, the sharded engine over the HIP ops, `Trainer(micro_batch=...)` on the tiny model against
itself and against the oracle, the RCCL call pattern on one GPU, and `train_loop` under KAI0_MICRO_BATCH.

Launch arithmetic of kai0_grad_accum (csrc/optim.hip), restated by `launch()` below from n and the pointers alone:
  head   = elements up to acc's first 16-byte boundary if the gradient reaches ITS vector boundary (8 B bf16, 16 B f32) at the same
           element, else n (everything scalar);  n4 = (n - head) // 4 vectors of four elements, rest = n - 4 n4 scalar elements
  blocks = min(ceil(n4 / 256), cap), at least min(max(ceil(rest / 256), 1), 4096);  cap = 2^22 without sumsq_out, 4096 with it
           (one partial per block in the 4096-float scratch buffer)
  every block takes ceil(n4 / blocks) consecutive vectors, a lane every 256th of them; the scalar elements are grid-strided.
A lane takes more than one vector beyond n4 = cap * 256: 2^22 elements with sumsq_out (covered: n = 2^22 + 4 * 333 + 3), 2^32 elements
without — above 2^28, so that case is skipped as the issue allows."""

import dataclasses as dc
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from streaming_refs import BF16, F32, F64, GUARD, SENTINEL  # noqa: E402
from test_streaming_kernels_gpu import DEV, P, call, rnd  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


def dev():
    return torch.device(DEV)


class Band:
    """A length-n view starting GUARD + off elements into a fresh (16-byte aligned) buffer of sentinels."""

    def __init__(self, n, dtype, off=0, init=None, fill=NAN):
        self.buf = torch.full((n + off + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD + off : GUARD + off + n]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        self.lo, self.hi = GUARD + off, GUARD + off + n
        if init is not None:
            self.t.copy_(init)
        else:
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.buf[: self.lo] == SENTINEL).all()) and bool((self.buf[self.hi :] == SENTINEL).all()), f"{what}: wrote outside its view"


def launch(n, acc_ptr, grad_ptr, gsz, sumsq):
    """(head, n4, rest, blocks, vectors per lane, scalar elements per lane) of kai0_grad_accum — see the module docstring."""
    head = min(((16 - acc_ptr % 16) % 16) // 4, n)
    if (grad_ptr + head * gsz) % (4 * gsz):
        head = n
    n4 = (n - head) // 4
    rest = n - 4 * n4
    blocks = max(min(-(-n4 // 256), 4096 if sumsq else 2**22), min(max(-(-rest // 256), 1), 4096))
    per = -(-n4 // blocks)
    stride = blocks * 256
    scalars = -(-head // stride) + -(-(rest - head) // stride) if head < n else -(-n // stride)
    return head, n4, rest, blocks, -(-per // 256), scalars


def sumsq_chain(n, acc_ptr, grad_ptr, gsz):
    """Longest chain of f32 roundings one partial goes through: per vector four squares (each rounds once) and four additions,
    per scalar element a square and an addition, 6 wave-shuffle steps, 4 wave partials; the finishing launch adds
    ceil(blocks / 256) partials per thread, 6 + 4 again, and `out[0] +=` is one more."""
    *_, blocks, vecs, scalars = launch(n, acc_ptr, grad_ptr, gsz, True)
    return 8 * vecs + 2 * scalars + 6 + 4 + -(-blocks // 256) + 6 + 4 + 1


# ================================================================================================ 1. kernel, bit-exact
OFFS = {"aligned": (0, 0), "one_in": (1, 1), "mixed": (1, 0)}  # (acc, grad) element offsets; mixed: no common head, the scalar form
SIZES = [(1, False), (255, False), (4099, False), (2**20 + 3, False), (4099, True), (2**22 + 4 * 333 + 3, True)]


@pytest.mark.skip(reason="without sumsq_out a lane takes a second vector only past 2^32 elements (2^22 blocks x 256 lanes x 4): above 2^28")
def test_grad_accum_second_vector_per_lane_without_sumsq():
    """The case the module docstring names: n = 2^32 + 4 * 333 + 3 with sumsq_out = NULL (26 GB of buffers)."""


@pytest.mark.parametrize("n,with_sumsq", SIZES)
@pytest.mark.parametrize("layout", list(OFFS))
@pytest.mark.parametrize("gdtype", [BF16, F32])
def test_grad_accum_is_one_f32_add(gdtype, layout, n, with_sumsq):
    """first = 1 into an accumulator full of NaN equals grad.float(); first = 0 equals torch's acc + grad.float(); bit for bit, for
    bf16 and f32 gradients, aligned views / both views one element in (a common scalar head, then 16-byte accesses) / the f32 view
    one element in and the gradient aligned (no common head: scalar throughout).  with_sumsq: the 4096-block form with its
    per-block partials (at 2^22 + 1335 elements a lane takes two vectors).  The elements around the views keep their bytes."""
    ao, go = OFFS[layout]
    g1 = Band(n, gdtype, go, init=rnd(n, dtype=gdtype, seed=1))
    g2 = Band(n, gdtype, go, init=rnd(n, dtype=gdtype, seed=2, scale=3.0))
    acc = Band(n, F32, ao)  # NaN
    out, scratch = Band(1, F32, fill=0.0), Band(4096, F32)
    head, n4, rest, blocks, vecs, _ = launch(n, acc.t.data_ptr(), g1.t.data_ptr(), g1.t.element_size(), with_sumsq)
    if n >= 4:
        assert head == {"aligned": 0, "one_in": 3, "mixed": n}[layout]
    if n > 2**22 and layout != "mixed":
        assert vecs == 2 and blocks == 4096
    so, sc = (P(out.t), P(scratch.t)) if with_sumsq else (None, None)
    call("kai0_grad_accum", P(acc.t), P(g1.t), int(gdtype == F32), n, 1, so, sc)
    torch.cuda.synchronize()
    acc.check("acc (first)")
    want1 = g1.t.float()
    assert torch.equal(acc.t, want1), f"first: {int((acc.t != want1).sum())} elements differ"
    call("kai0_grad_accum", P(acc.t), P(g2.t), int(gdtype == F32), n, 0, so, sc)
    torch.cuda.synchronize()
    want2 = want1 + g2.t.float()
    assert torch.equal(acc.t, want2), f"add: {int((acc.t != want2).sum())} elements differ"
    for b, what in ((acc, "acc"), (g1, "grad 1"), (g2, "grad 2"), (out, "sumsq_out"), (scratch, "scratch")):
        b.check(what)
    assert torch.equal(g2.t, rnd(n, dtype=gdtype, seed=2, scale=3.0))  # the gradient is only read
    if with_sumsq:
        assert float(out.t[0]) > 0 and int(torch.isnan(scratch.t[:blocks]).sum()) == 0
        assert bool(torch.isnan(scratch.t[blocks:]).all())  # partials beyond the grid are not touched
    else:
        assert float(out.t[0]) == 0.0 and bool(torch.isnan(scratch.t).all())


# ================================================================================================ 2. fused sum of squares
@pytest.mark.parametrize("layout", list(OFFS))
@pytest.mark.parametrize("gdtype,n", [(BF16, 2**22 + 4 * 333 + 3), (F32, 2**20 + 3), (BF16, 255)])
def test_grad_accum_fused_sumsq(gdtype, n, layout):
    """sumsq_out[0] += sum(acc_new^2) against the float64 sum over the stored new accumulator; all addends non-negative, so the
    bound is (2^-23 + L 2^-24) * ref with L the longest chain of f32 roundings (sumsq_chain above, from n and the pointers, not from
    the kernel's output) — test_sumsq_past_the_grid_cap's form.  Two calls into one `out` give exactly twice the result (fixed-order
    partials: reproducible); `out` and `scratch` sit in guard bands."""
    ao, go = OFFS[layout]
    grad = Band(n, gdtype, go, init=rnd(n, dtype=gdtype, seed=3))
    acc0 = rnd(n, dtype=F32, seed=4, scale=2.0)
    want = acc0 + grad.t.float()
    ref = float((want.to(F64) ** 2).sum())
    res = []
    for _ in range(2):
        acc = Band(n, F32, ao, init=acc0)
        L = sumsq_chain(n, acc.t.data_ptr(), grad.t.data_ptr(), grad.t.element_size())
        bnd = (2.0**-23 + L * 2.0**-24) * ref
        out, scratch = Band(1, F32, fill=0.0), Band(4096, F32)
        call("kai0_grad_accum", P(acc.t), P(grad.t), int(gdtype == F32), n, 0, P(out.t), P(scratch.t))
        torch.cuda.synchronize()
        for b, what in ((acc, "acc"), (out, "sumsq_out"), (scratch, "scratch")):
            b.check(what)
        assert torch.equal(acc.t, want)
        res.append(float(out.t[0]))
    r = abs(res[0] - ref) / bnd
    print(f"worst error/bound grad_accum sumsq {gdtype} n={n} {layout}: {r:.3f} (chain {L})")
    assert r <= 1.0, f"{res[0]!r} vs {ref!r}: error/bound {r:.3f}"
    assert res[1] == res[0]
    # accumulates into out[0]: a second call on the same inputs (first = 1, the same new accumulator) adds the same number again
    acc, out, scratch = Band(n, F32, ao), Band(1, F32, fill=0.0), Band(4096, F32)
    for _ in range(2):
        call("kai0_grad_accum", P(acc.t), P(want), 1, n, 1, P(out.t), P(scratch.t))
    one = Band(1, F32, fill=0.0)
    call("kai0_grad_accum", P(acc.t), P(want), 1, n, 1, P(one.t), P(scratch.t))
    torch.cuda.synchronize()
    assert float(out.t[0]) == float(one.t[0] + one.t[0]) and float(one.t[0]) > 0
    out.check("sumsq_out"), scratch.check("scratch")


# ================================================================================================ 3. argument checks
def test_grad_accum_argument_checks():
    from kai0_amd import _lib, optim

    acc, grad, out, scratch = (torch.zeros(16, device=DEV) for _ in range(4))
    for args, msg in (((None, P(grad), 1, 16, 1, None, None), "null buffer"), ((P(acc), None, 1, 16, 0, None, None), "null buffer"),
                      ((P(acc), P(grad), 1, 16, 0, P(out), None), "scratch")):  # fmt: skip
        with pytest.raises(_lib.Kai0HipError, match=msg):
            call("kai0_grad_accum", *args)
    call("kai0_grad_accum", None, None, 1, 0, 1, None, None)  # n <= 0: nothing to do, nothing checked
    call("kai0_grad_accum", P(acc), P(grad), 1, 16, 0, None, P(scratch))  # a scratch buffer without sumsq_out is simply unused
    g = torch.arange(16, device=DEV, dtype=F32).to(BF16)
    optim.grad_accum_(acc, g, first=True, sumsq_out=out)
    torch.cuda.synchronize()
    assert torch.equal(acc, g.float()) and float(out[0]) == float((g.float() ** 2).sum())


# ================================================================================================ 4. engine over the HIP ops
class _Net(torch.nn.Module):
    """f32 throughout: a 1500-row table (row-sparse AdamW path) and two linear layers."""

    def __init__(self, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.table = torch.nn.Parameter(torch.randn(1500, 72) * 0.05)
        self.l1, self.l2 = torch.nn.Linear(72, 40), torch.nn.Linear(40, 8)

    def forward(self, tok):
        return self.l2(torch.tanh(self.l1(self.table[tok]))).pow(2).mean()


def _net_engine(ema, clip):
    from kai0_amd.sharded import HipShardOps, ShardedDataParallel

    class Counting(HipShardOps):
        rows = accum = 0

        def adamw_rows(self, *a, **kw):
            self.rows += 1
            super().adamw_rows(*a, **kw)

        def adamw_rows_ema(self, *a, **kw):
            self.rows += 1
            super().adamw_rows_ema(*a, **kw)

        def grad_accum(self, *a, **kw):
            self.accum += 1
            super().grad_accum(*a, **kw)

    model = _Net(seed=3).to(dev())
    model.table._kai0_grad_accumulates = True
    eng = ShardedDataParallel(list(model.named_parameters()), world_size=1, rank=0, ops=Counting(), weight_decay=1e-10,
                              max_grad_norm=clip, bucket_bytes=4096, ema_decay=ema)  # fmt: skip
    assert len(eng.buckets) >= 3
    return model, eng


def _tokens(step):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randperm(1000, generator=g)[: 20 + 5 * step].to(dev()) for _ in range(2)]  # (unique ids: no duplicate-index adds)


@pytest.mark.parametrize("ema", [None, 0.99])
def test_engine_accumulation_through_the_hip_ops_is_bit_exact(ema):
    """A: loss(x1)/2 backward, end_micro_batch(), loss(x2)/2 backward, step.  B: (loss(x1)/2 + loss(x2)/2).backward(), step.  Both
    add the two gradients with one f32 add per element (A: kai0_grad_accum, B: autograd), which is commutative: after 4 steps
    parameters, masters, moments and EMA are bit-identical (dense, row-sparse and both EMA forms read `acc` as an f32 gradient)."""
    (ma, ea), (mb, eb) = _net_engine(ema, None), _net_engine(ema, None)
    for step in range(4):
        x1, x2 = _tokens(step)
        ea.begin_step()
        (ma(x1) / 2).backward()
        ea.end_micro_batch()
        (ma(x2) / 2).backward()
        ea.step(2.5e-5)
        eb.begin_step()
        (mb(x1) / 2 + mb(x2) / 2).backward()
        eb.step(2.5e-5)
    torch.cuda.synchronize()
    assert ea.ops.rows == eb.ops.rows == 4 and ea.ops.accum == 8 * len(ea.buckets) and eb.ops.accum == 0
    assert ea.step_count == eb.step_count == 4
    for (k, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p, q), k
    for a, b in zip(ea.buckets, eb.buckets):
        for key in ("master", "exp_avg", "exp_avg_sq") + (("ema",) if ema is not None else ()):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert a.acc.dtype == F32 and a.acc.numel() == a.shard and not hasattr(b, "acc")
        assert torch.equal(a.acc, b.grad_shard) or a.params[0] is ma.table  # (the table's flat gradient is re-zeroed after the step)
    assert float(ea.buckets[0].exp_avg.abs().sum()) > 0 and not torch.equal(ma.table, _Net(seed=3).table.to(dev()))


def test_engine_accumulated_norm_is_the_norm_of_the_summed_gradient():
    """With clipping the two engines take their sum of squares over different buffers and in different orders (A: fused into the
    last kai0_grad_accum over `acc`; B: kai0_sumsq over the f32 gradient shard) of the SAME values: each is within
    (2^-23 + L 2^-24) of the exact sum (test 2's bound; + 1 per bucket for `out[0] +=`), so the norms (a square root: half the
    relative error, and one more rounding of at most 2^-23 each) differ by at most (L_A + L_B) / 2 * 2^-24 + 3 * 2^-23 relative."""
    import streaming_refs as R

    (ma, ea), (mb, eb) = _net_engine(None, 1e-6), _net_engine(None, 1e-6)
    x1, x2 = _tokens(0)
    (ma(x1) / 2).backward()
    ea.end_micro_batch()
    (ma(x2) / 2).backward()
    na = float(ea.step(2.5e-5))
    (mb(x1) / 2 + mb(x2) / 2).backward()
    nb = float(eb.step(2.5e-5))
    exact = float(sum((b.acc.to(F64) ** 2).sum() for b in ea.buckets) ** 0.5)
    nbk = len(ea.buckets)
    la = max(sumsq_chain(b.shard, b.acc.data_ptr(), b.grad_shard.data_ptr(), 4) for b in ea.buckets) + nbk
    lb = max(R.sumsq_chain(b.shard, True) for b in eb.buckets) + nbk
    bnd = (la + lb) / 2 * 2.0**-24 + 3 * 2.0**-23
    print(f"accumulated norm {na!r} vs summed-loss norm {nb!r} (exact {exact!r}): relative difference {abs(na - nb) / exact:.3e}, bound {bnd:.3e}")
    assert na > 1e-6 and abs(na - nb) <= bnd * exact and abs(na - exact) <= bnd * exact
    assert float(ea._coef) < 1.0  # it clips


# ================================================================================================ 5. model, bit-exact
def _tiny_trainer(seed=0, **kw):
    from tiny import build_pair

    from kai0_amd.train import Trainer

    model, oracle, pcfg, ocfg = build_pair(dev(), seed=seed, std=0.08)
    model.train()
    base = dict(world_size=1, rank=0, peak_lr=1e-3, warmup_steps=0, decay_steps=10, end_lr=1e-3, clip_norm=1.0, bucket_bytes=1 << 16)
    base.update(kw)
    return Trainer(model, **base), oracle, ocfg


def _batch(ocfg, B, seed=0):
    from tiny import obs_to

    from oracle.pi0_oracle import synthetic_batch

    obs, actions, noise, time = synthetic_batch(ocfg, B, seed=seed)
    return obs, (obs_to(obs, dev()), actions.to(dev()), noise.to(dev()), time.to(dev())), (actions, noise, time)


def _engine_state(tr):
    tr.params_ready()
    return [p.detach().clone() for p in tr.model.parameters()] + [getattr(b, k).clone() for b in tr.engine.buckets
                                                                   for k in ("master", "exp_avg", "exp_avg_sq")]  # fmt: skip


def _first_sample_twice(obs):
    def dup(v):
        if isinstance(v, dict):
            return {k: dup(x) for k, x in v.items()}
        return torch.cat([v[:1], v[:1]]) if isinstance(v, torch.Tensor) else v

    return type(obs)(**{k: dup(v) for k, v in vars(obs).items()})


def test_two_identical_samples_as_two_micro_batches_equal_the_one_sample_step():
    """Batch of two IDENTICAL samples (same noise and time) as micro_batch = 1 against the step on the one sample, no clipping: the
    losses carry 1/2, a power of two, which commutes with every rounding of the backward (linear in the upstream gradient), and
    g/2 + g/2 = g exactly — losses, parameters, masters and moments are bit-identical over 3 steps."""
    from kai0_amd.preprocessing import slice_observation

    split, _, ocfg = _tiny_trainer(micro_batch=1, clip_norm=None)
    single, _, _ = _tiny_trainer(clip_norm=None)
    assert split.micro_batch == 1 and single.micro_batch is None
    for step in range(3):
        _, (gobs, actions, noise, time), _ = _batch(ocfg, 2, seed=50 + step)
        one = (slice_observation(gobs, 0, 1), actions[:1], noise[:1], time[:1])
        twice = (_first_sample_twice(gobs), *(torch.cat([t[:1], t[:1]]) for t in (actions, noise, time)))
        la, lb = split.train_step(*twice), single.train_step(*one)
        torch.cuda.synchronize()
        assert la.dim() == 0 and torch.equal(la, lb), (step, float(la), float(lb))
    assert split.global_step == single.global_step == 3 and split.engine.step_count == 3
    for i, (a, b) in enumerate(zip(_engine_state(split), _engine_state(single))):
        assert torch.equal(a, b), i
    assert not any(hasattr(b, "acc") for b in single.engine.buckets)


# ================================================================================================ 6. model, against the oracle
@pytest.fixture(scope="module")
def oracle_grads():
    """The fp32 oracle's autograd gradient of the full-batch (B = 4) mean loss, and the unsplit HIP gradient (plain autograd)."""
    import copy

    from tiny import build_pair

    model, oracle, _, ocfg = build_pair(dev(), seed=0, std=0.08)
    obs, gbatch, (actions, noise, time) = _batch(ocfg, 4)
    o32 = copy.deepcopy(oracle)
    o32.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    o32(obs, actions, noise, time).mean().backward()
    go = {n: (None if p.grad is None else p.grad.clone()) for n, p in o32.named_parameters()}
    norm = float(torch.sqrt(sum(g.double().pow(2).sum() for g in go.values() if g is not None)))
    model.train()
    model(*gbatch[:2], noise=gbatch[2], time=gbatch[3]).mean().backward()
    gm = {n: (None if p.grad is None else p.grad.detach().float().cpu()) for n, p in model.named_parameters()}
    return dict(oracle=go, hip=gm, norm=norm, batch=gbatch)


@pytest.mark.parametrize("micro", [2, 1])
def test_accumulated_gradient_matches_the_oracle(oracle_grads, micro):
    """B = 4 as 2 x 2 and as 4 x 1: every parameter's slice of `acc` after step() against the oracle's gradient of the full-batch
    mean loss at per-parameter rel-L2 <= 0.025 with the small-norm exclusions (test_backward_matches_oracle_autograd's bound for the
    unsplit gradient), against the unsplit HIP gradient at <= 0.05 (triangle inequality), the norm within 3e-2 (the trajectory
    test's bound)."""
    tr, _, _ = _tiny_trainer(micro_batch=micro)
    gobs, actions, noise, time = oracle_grads["batch"]
    loss = tr.train_step(gobs, actions, noise, time)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and tr.engine.step_count == 1
    go, gm = oracle_grads["oracle"], oracle_grads["hip"]
    table, bad, checked = [], [], 0
    for b in tr.engine.buckets:
        for p, o, n in zip(b.params, b.offsets, b.names):
            got = b.acc[o : o + p.numel()].view(p.shape).cpu()
            g = go[n]
            if g is None:
                assert float(got.abs().max()) == 0.0, f"{n} must not receive a gradient"
                continue
            if float(g.norm()) < 1e-8:
                assert float(got.norm()) < 1e-4, n
                continue
            r = float((got - g).norm() / (g.norm() + 1e-12))
            rh = float((got - gm[n]).norm() / (gm[n].norm() + 1e-12))
            table.append((r, rh, n))
            checked += 1
            if r >= 0.025 or rh >= 0.05:
                bad.append((r, rh, n))
    table.sort(reverse=True)
    print(f"micro_batch={micro}: {checked} gradients; worst rel-L2 vs oracle {table[0][0]:.3e} ({table[0][2]}), "
          f"worst vs unsplit HIP {max(t[1] for t in table):.3e}")  # fmt: skip
    gn = float(tr.last_grad_norm)
    print(f"micro_batch={micro}: grad norm {gn:.6f} vs oracle {oracle_grads['norm']:.6f}: relative {abs(gn - oracle_grads['norm']) / oracle_grads['norm']:.3e}")
    assert not bad, f"{len(bad)} gradient mismatches, worst: {sorted(bad, reverse=True)[:5]}"
    assert checked > 100
    assert abs(gn - oracle_grads["norm"]) < 3e-2 * oracle_grads["norm"]


# ================================================================================================ 7. collectives on one GPU
@pytest.mark.parametrize("mode", ["zero2", "fsdp"])
def test_accumulating_trainer_with_rccl_collectives_equals_the_collective_free_one(mode, monkeypatch):
    """test_trainer_with_rccl_collectives_equals_collective_free_engine's pattern (a 1-rank RCCL group, KAI0_FORCE_COLLECTIVES=1)
    with micro_batch = half the batch: every micro-batch is reduce-scattered, only the shard is accumulated; 3 steps bit-identical
    to the collective-free accumulating trainer.  fsdp: the full parameter buffers are released between micro-batches."""
    import torch.distributed as dist

    resident = []

    def run(collective):
        tr, _, ocfg = _tiny_trainer(seed=3, mode=mode, micro_batch=1)
        eng = tr.engine
        assert eng.collectives == collective and eng.mode == (mode if collective else "zero2")
        inner = eng.end_micro_batch

        def end_micro_batch():
            inner()
            if collective:
                resident.append([eng.buckets[bi].resident for ids in eng.groups[1:] for bi in ids])

        eng.end_micro_batch = end_micro_batch
        _, batch, _ = _batch(ocfg, 2)
        losses = [float(tr.train_step(*batch)) for _ in range(3)]
        torch.cuda.synchronize()
        assert all(b.acc.numel() == b.shard for b in eng.buckets)
        return losses, _engine_state(tr), float(tr.last_grad_norm)

    base = run(False)
    monkeypatch.setenv("KAI0_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29631")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    try:
        got = run(True)
    finally:
        dist.destroy_process_group()
    assert got[0] == base[0] and got[2] == base[2]
    assert all(torch.equal(a, b) for a, b in zip(got[1], base[1]))
    assert len(resident) == 3 and len(resident[0]) > 2
    assert all(r == (mode != "fsdp") for rs in resident for r in rs)


# ================================================================================================ 8. train_loop
@pytest.mark.timeout(600)
def test_train_loop_debug_pi05_with_micro_batches_resumes_exactly(tmp_path, monkeypatch):
    """`train_loop(get_config("debug_pi05"))` (batch 2) under KAI0_MICRO_BATCH=1: the start-up line names the switch, and the run
    stopped after 2 steps and resumed to 4 logs the uninterrupted run's steps 2 and 3 exactly
    (test_train_loop_debug_pi05_resume_is_exact's criteria)."""
    from kai0_amd import training_config as tc
    from kai0_amd.train import train_loop

    monkeypatch.setenv("KAI0_MICRO_BATCH", "1")
    lines = []
    base = dc.replace(tc.get_config("debug_pi05"), checkpoint_base_dir=str(tmp_path / "ckpt"), assets_base_dir=str(tmp_path / "assets"),
                      num_workers=0, num_train_steps=4, log_interval=1, save_interval=100,
                      lr_schedule=tc.CosineDecaySchedule(warmup_steps=2, peak_lr=1e-3, decay_steps=10, decay_lr=1e-4))  # fmt: skip
    full = train_loop(dc.replace(base, exp_name="full", overwrite=True), log=lines.append)
    assert [r["step"] for r in full] == list(range(4)) and all(r["loss"] == r["loss"] for r in full)
    assert sum("micro_batch=1 (KAI0_MICRO_BATCH" in l for l in lines) == 1, lines
    assert sorted(os.listdir(tmp_path / "ckpt" / "debug_pi05" / "full" / "4")) == ["metadata.pt", "model.safetensors", "optimizer.pt"]
    part = train_loop(dc.replace(base, exp_name="cut", num_train_steps=2, overwrite=True))
    assert [r["loss"] for r in part] == [r["loss"] for r in full[:2]]
    rest = train_loop(dc.replace(base, exp_name="cut", overwrite=False, resume=True))
    assert [r["step"] for r in rest] == [2, 3]
    for a, b in zip(rest, full[2:]):
        assert a["loss"] == b["loss"] and a["grad_norm"] == b["grad_norm"] and a["learning_rate"] == b["learning_rate"], (a, b)
