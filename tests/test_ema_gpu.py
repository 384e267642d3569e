"""Parameter EMA on the MI355X: the fused kernels `kai0_adamw_ema` / `kai0_adamw_rows_ema` against `kai0_adamw`, and the Trainer
with an EMA decay on the tiny model (training unperturbed, `ema_weights()` around `sample_actions`, `model_ema.safetensors`).

Bound of one EMA step (derived in tests/test_ema_cpu.py's docstring): against e + (1 - d)(p - e) evaluated in float64 from the same
f32 inputs (d as the f32 the kernel receives), |e' - ref| <= 2^-21 * max(|e|, |p|) elementwise; multi-step runs are compared
step by step (previous EMA as stored, new master as stored)."""

import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
KW = dict(beta1=0.9, beta2=0.95, eps=1e-8)


def dev():
    return torch.device("cuda:0")


def assert_ema_step(prev, master, new, d):
    d32 = float(np.float32(d))
    ref = prev.double() + (1.0 - d32) * (master.double() - prev.double())
    bound = 2.0**-21 * torch.maximum(prev.abs(), master.abs()).double()
    err = (new.double() - ref).abs()
    print(f"    ema step d={d}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.max()))


def _view(n, dtype, off, gen, std=None, like=None):
    """A length-n view starting `off` elements into a fresh (16-byte aligned) allocation."""
    buf = torch.zeros(n + off + 8, dtype=dtype, device=dev())
    v = buf[off : off + n]
    if like is not None:
        v.copy_(like)
    elif std is not None:
        v.copy_(torch.randn(n, device=dev(), generator=gen) * std)
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    return v


# ---------------------------------------------------------------------------------------------- 8. kai0_adamw_ema
@pytest.mark.parametrize("layout", ["aligned", "one_in", "mixed"])
@pytest.mark.parametrize("pdtype", [F32, BF16])
@pytest.mark.parametrize("gdtype", [F32, BF16])
def test_adamw_ema_is_adamw_plus_the_average(gdtype, pdtype, layout):
    """master / m / v / model copy bit-identical to kai0_adamw on cloned inputs, EMA within the bound of the float64 expression: every
    (grad, param) dtype pair; n = 1, 255, 4099, 2^20 + 3; 16-byte aligned buffers, views starting one element in (a shard slice: a common
    scalar head, then 16-byte accesses) and f32 streams one element in with aligned 16-bit ones (no common head: the scalar form; for
    f32 grad and param this is `one_in` again); with and without a clip coefficient; decays 0.99, 0.999 and 0."""
    from kai0_amd import optim

    gen = torch.Generator(device=dev()).manual_seed(11)
    coef = torch.tensor([0.37], device=dev())
    off32 = 0 if layout == "aligned" else 1
    off = lambda dt: off32 if (dt == F32 or layout != "mixed") else 0  # noqa: E731
    for n in (1, 255, 4099, 2**20 + 3):
        master0 = _view(n, F32, off32, gen, std=0.02)
        m0, v0 = _view(n, F32, off32, gen), _view(n, F32, off32, gen)
        param0 = _view(n, pdtype, off(pdtype), gen, like=master0)
        # moments from one earlier step, so nothing is trivially zero
        g_prev = _view(n, gdtype, off(gdtype), gen, std=1.0)
        optim.adamw_step_(master0, m0, v0, g_prev, param0, lr=1e-3, wd=1e-2, step=1, clip_coef=None, **KW)
        ema0 = _view(n, F32, off32, gen, like=master0 + torch.randn(n, device=dev(), generator=gen) * 1e-3)
        grad = _view(n, gdtype, off(gdtype), gen, std=1.0)
        for clip in (None, coef):
            for d in (0.99, 0.999, 0.0):
                ref = [_view(n, F32, off32, gen, like=t) for t in (master0, m0, v0)] + [_view(n, pdtype, off(pdtype), gen, like=param0)]
                got = [_view(n, F32, off32, gen, like=t) for t in (master0, m0, v0)] + [_view(n, pdtype, off(pdtype), gen, like=param0)]
                ema = _view(n, F32, off32, gen, like=ema0)
                guard = ema.clone()
                optim.adamw_step_(ref[0], ref[1], ref[2], grad, ref[3], lr=1e-3, wd=1e-2, step=2, clip_coef=clip, **KW)
                optim.adamw_ema_step_(got[0], got[1], got[2], ema, grad, got[3], lr=1e-3, wd=1e-2, step=2, ema_decay=d, clip_coef=clip, **KW)
                for a, b, what in zip(got, ref, ("master", "m", "v", "param")):
                    assert torch.equal(a, b), (what, n, d, clip is not None)
                assert not torch.equal(got[0], master0)
                print(f"  n={n} clip={clip is not None}")
                assert_ema_step(guard, got[0], ema, d)
        # the fixed point: ema == master, zero gradient, zero moments (wd rounding away) -> the EMA comes back bit-identical
        fp = [_view(n, F32, off32, gen, like=master0), _view(n, F32, off32, gen), _view(n, F32, off32, gen)]
        fp_param = _view(n, pdtype, off(pdtype), gen, like=master0)
        fp_ema = _view(n, F32, off32, gen, like=master0)
        optim.adamw_ema_step_(fp[0], fp[1], fp[2], fp_ema, _view(n, gdtype, off(gdtype), gen), fp_param, lr=2.5e-5, wd=1e-10, step=2,
                              ema_decay=0.99, clip_coef=coef, **KW)  # fmt: skip
        assert torch.equal(fp_ema, master0) and torch.equal(fp[0], master0) and not bool(fp[1].any()) and not bool(fp[2].any())


def test_adamw_ema_leaves_its_neighbours_alone():
    """Odd length, views one element in: the elements before and after the views (head / tail handling) keep their bytes."""
    from kai0_amd import optim

    n = 4099
    bufs = {k: torch.full((n + 9,), 7.0, dtype=dt, device=dev()) for k, dt in (("master", F32), ("m", F32), ("v", F32), ("ema", F32),
                                                                               ("grad", BF16), ("param", BF16))}  # fmt: skip
    vs = {k: b[1 : 1 + n] for k, b in bufs.items()}
    vs["grad"].fill_(1.0)  # (values chosen so that no updated element lands on 7.0 again)
    optim.adamw_ema_step_(vs["master"], vs["m"], vs["v"], vs["ema"], vs["grad"], vs["param"], lr=1.0, wd=1e-2, step=1, ema_decay=0.9,
                          clip_coef=None, **KW)  # fmt: skip
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert float(b[0]) == 7.0 and bool((b[1 + n :] == 7.0).all()), k
        assert k == "grad" or not bool((b[1 : 1 + n] == 7.0).any()), k


def test_adamw_ema_argument_checks():
    from kai0_amd import _lib, optim

    t = lambda dt=F32: torch.zeros(16, dtype=dt, device=dev())  # noqa: E731
    for bad in (1.0, -0.01):
        with pytest.raises(_lib.Kai0HipError, match="ema_decay"):
            optim.adamw_ema_step_(t(), t(), t(), t(), t(BF16), t(BF16), lr=1e-3, wd=0.0, step=1, ema_decay=bad, **KW)
    with pytest.raises(_lib.Kai0HipError, match="null ema"):
        _lib.call("kai0_adamw_ema", t().data_ptr(), t().data_ptr(), t().data_ptr(), None, t().data_ptr(), 1, t().data_ptr(), 1, 16,
                  1e-3, 0.9, 0.95, 1e-8, 0.0, 0.1, 0.05, 0.99, None, None)  # fmt: skip


# ------------------------------------------------------------------------------------------ 9. kai0_adamw_rows_ema
def test_adamw_rows_ema_is_bit_identical_to_the_dense_ema_update():
    """4096 x 2048 table, bf16 gradient in 64 rows: all five outputs equal kai0_adamw_ema's.  Rows without gradient and with a clear
    flag hold ema == master and zero moments (what the host guarantees for them) and keep their EMA bytes; the 64 gradient rows have
    ema != master; 16 more rows have no gradient but a set flag (moments nonzero, ema != master) and must be updated too."""
    from kai0_amd import optim

    rows, rl = 4096, 2048
    n = rows * rl
    gen = torch.Generator(device=dev()).manual_seed(5)
    perm = torch.randperm(rows, device=dev(), generator=gen)
    hot, flagged = perm[:64], perm[64:80]
    master = torch.randn(rows, rl, device=dev(), generator=gen) * 0.02
    master = master.to(BF16).float()
    ema, m, v = master.clone(), torch.zeros_like(master), torch.zeros_like(master)
    for idx in (hot, flagged):
        ema[idx] += torch.randn(idx.numel(), rl, device=dev(), generator=gen) * 1e-3
    m[flagged] = torch.randn(16, rl, device=dev(), generator=gen) * 1e-2
    v[flagged] = torch.rand(16, rl, device=dev(), generator=gen) * 1e-4
    grad = torch.zeros(rows, rl, device=dev())
    grad[hot] = torch.randn(64, rl, device=dev(), generator=gen)
    grad = grad.to(BF16).reshape(-1)
    active = torch.zeros(rows, dtype=torch.uint8, device=dev())
    active[flagged] = 1
    coef = torch.tensor([0.37], device=dev())
    dense = [t.clone().reshape(-1) for t in (master, m, v, ema)] + [master.to(BF16).reshape(-1)]
    sparse = [t.clone().reshape(-1) for t in (master, m, v, ema)] + [master.to(BF16).reshape(-1)]
    kw = dict(lr=2.5e-5, wd=1e-10, step=3, ema_decay=0.99, clip_coef=coef, **KW)
    optim.adamw_ema_step_(dense[0], dense[1], dense[2], dense[3], grad, dense[4], **kw)
    optim.adamw_rows_ema_step_(sparse[0], sparse[1], sparse[2], sparse[3], grad, sparse[4], rl, active, **kw)
    for a, b, what in zip(sparse, dense, ("master", "m", "v", "ema", "param")):
        assert torch.equal(a, b), what
    busy = torch.zeros(rows, dtype=torch.bool, device=dev())
    busy[hot] = True
    busy[flagged] = True
    assert torch.equal(active.bool(), busy)  # the kernel flagged the gradient rows
    assert torch.equal(sparse[3].view(rows, rl)[~busy], ema[~busy]) and torch.equal(sparse[0].view(rows, rl)[~busy], master[~busy])
    assert bool((sparse[3].view(rows, rl)[busy] != ema[busy]).any(1).all())
    assert_ema_step(ema[busy], sparse[0].view(rows, rl)[busy], sparse[3].view(rows, rl)[busy], 0.99)
    with pytest.raises(Exception, match="does not round away"):
        optim.adamw_rows_ema_step_(sparse[0], sparse[1], sparse[2], sparse[3], grad, sparse[4], rl, active, lr=1e-3, wd=1e-2, step=4,
                                   ema_decay=0.99, clip_coef=coef, **KW)  # fmt: skip
    # rows that are not a multiple of four elements long, views one element in: the scalar form, same result
    rows2, rl2 = 1030, 67
    n2 = rows2 * rl2
    base = [torch.zeros(n2 + 1, device=dev()) for _ in range(8)] + [torch.zeros(n2 + 1, device=dev(), dtype=BF16) for _ in range(3)]
    d4, s4, (pd, ps, g2) = [b[1:] for b in base[:4]], [b[1:] for b in base[4:8]], [b[1:] for b in base[8:]]
    p2 = torch.randn(n2, device=dev(), generator=gen) * 0.02
    hot2 = torch.randperm(rows2, device=dev(), generator=gen)[:20]
    gg = torch.zeros(rows2, rl2, device=dev())
    gg[hot2] = torch.randn(20, rl2, device=dev(), generator=gen)
    g2.copy_(gg.reshape(-1))
    for st, par in ((d4, pd), (s4, ps)):
        st[0].copy_(p2), st[3].copy_(p2), par.copy_(p2)
        st[3].view(rows2, rl2)[hot2] += 1e-3
    act2 = torch.zeros(rows2, dtype=torch.uint8, device=dev())
    optim.adamw_ema_step_(d4[0], d4[1], d4[2], d4[3], g2, pd, **kw)
    optim.adamw_rows_ema_step_(s4[0], s4[1], s4[2], s4[3], g2, ps, rl2, act2, **kw)
    assert all(torch.equal(a, b) for a, b in zip(s4 + [ps], d4 + [pd])) and int(act2.sum()) == 20
    # small tables, aligned (off = 0) and as views one element in (off = 1: scalar scan, scalar update).  (19, 12): scalar scan, vector
    # update; (19, 6): scalar throughout; (5, 2056): a second trip of the 2048-element scan stride and of the 1024-element update stride.
    # Every third row is idle (zeros and -0.0 for a gradient, ema == master, zero moments): it keeps its bytes and its clear flag.
    for rows3, rl3 in ((37, 8), (19, 12), (19, 6), (5, 2056)):
        for off in (0, 1):
            n3 = rows3 * rl3
            live = torch.tensor([i % 3 != 1 for i in range(rows3)], device=dev())
            p3 = (torch.randn(rows3, rl3, device=dev(), generator=gen) * 0.02).to(BF16).float()
            e3 = p3.clone()
            e3[live] += 1e-3
            g3 = torch.randn(rows3, rl3, device=dev(), generator=gen)
            g3[~live] = 0
            g3[~live, ::2] = -0.0
            g3 = _view(n3, BF16, off, gen, like=g3.reshape(-1))
            init = [p3.reshape(-1), torch.zeros(n3, device=dev()), torch.zeros(n3, device=dev()), e3.reshape(-1), p3.reshape(-1).to(BF16)]
            d3, s3 = ([_view(n3, t.dtype, off, gen, like=t) for t in init] for _ in range(2))
            act3 = torch.zeros(rows3, dtype=torch.uint8, device=dev())
            optim.adamw_step_(d3[0], d3[1], d3[2], g3, d3[4], ema=d3[3], **kw)
            optim.adamw_step_(s3[0], s3[1], s3[2], g3, s3[4], ema=s3[3], row_len=rl3, row_active=act3, **kw)
            for a, b, t, what in zip(s3, d3, init, ("master", "m", "v", "ema", "param")):
                assert torch.equal(a, b), (what, rows3, rl3, off)
                assert torch.equal(a.view(rows3, rl3)[~live], t.view(rows3, rl3)[~live]), (what, rows3, rl3, off)
            assert bool((s3[3].view(rows3, rl3)[live] != e3[live]).any(1).all())
            assert torch.equal(act3.bool(), live), (rows3, rl3, off)


# -------------------------------------------------------------------------------------------------- 10. Trainer
def _trainer(ema_decay, **kw):
    from tiny import build_pair

    from kai0_amd.train import Trainer

    model, _, pcfg, ocfg = build_pair(dev(), seed=3, std=0.08)
    model.train()
    tr = Trainer(model, world_size=1, rank=0, peak_lr=2e-3, warmup_steps=2, decay_steps=10, end_lr=2e-4, clip_norm=1.0,
                 bucket_bytes=1 << 16, ema_decay=ema_decay, **kw)  # fmt: skip
    return tr, pcfg, ocfg


def _batch(ocfg, seed):
    from tiny import obs_to

    from oracle.pi0_oracle import synthetic_batch

    obs, actions, noise, time = synthetic_batch(ocfg, 2, seed=seed)
    return obs_to(obs, dev()), actions.to(dev()), noise.to(dev()), time.to(dev())


def test_trainer_with_ema_trains_exactly_as_without_and_averages_every_step():
    tr, _, ocfg = _trainer(0.99)
    plain, _, _ = _trainer(None)
    assert len(tr.engine.buckets) > 2 and not hasattr(plain.engine.buckets[0], "ema")
    assert tr.engine.optimizer_state_bytes() * 3 == plain.engine.optimizer_state_bytes() * 4
    for step in range(5):
        prev = [b.ema.clone() for b in tr.engine.buckets]
        batch = _batch(ocfg, 100 + step)
        la, lb = tr.train_step(*batch), plain.train_step(*batch)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(tr.last_grad_norm, plain.last_grad_norm), step
        for b, e0 in zip(tr.engine.buckets, prev):
            assert_ema_step(e0, b.master, b.ema, 0.99)
    tr.params_ready(), plain.params_ready()
    for (k, p), (_, q) in zip(tr.model.named_parameters(), plain.model.named_parameters()):
        assert torch.equal(p, q), k
    for a, b in zip(tr.engine.buckets, plain.engine.buckets):
        assert torch.equal(a.master, b.master) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
        assert not torch.equal(a.ema, a.master)


def test_engine_row_sparse_path_with_ema_on_the_hip_kernels():
    """The sharded engine over HipShardOps on a table with >= 1024 rows: whole rows through kai0_adamw_rows_ema, the rest through
    kai0_adamw_ema; parameters, masters, moments and EMA after 5 steps bit-identical to the all-dense engine, then weights written
    into idle rows + sync_master_from_params(): their EMA moves by (1 - d) of the jump (the widened activity flag)."""
    from test_sharded_cpu import _Embed

    from kai0_amd.sharded import HipShardOps, ShardedDataParallel

    class Counting(HipShardOps):
        rows_calls = 0

        def adamw_rows_ema(self, *a, **kw):
            Counting.rows_calls += 1
            super().adamw_rows_ema(*a, **kw)

    rows, dim, d = 1500, 72, 0.99
    idle = torch.tensor([1210, 1300, 1499], device=dev())
    res = {}
    for sparse in (True, False):
        model = _Embed(rows, dim, seed=3).to(dev())
        model.table._kai0_grad_accumulates = True
        eng = ShardedDataParallel(list(model.named_parameters()), world_size=1, rank=0, ops=Counting(), weight_decay=1e-10,
                                  bucket_bytes=1 << 30, ema_decay=d)  # fmt: skip
        eng._sparse_rows = sparse
        Counting.rows_calls = 0
        g = torch.Generator().manual_seed(100)
        for step in range(5):
            eng.begin_step()
            model(torch.randint(0, 1000, (20 + 5 * step,), generator=g).to(dev())).backward()
            eng.step(2.5e-5)
        assert Counting.rows_calls == (5 if sparse else 0)
        b = eng.buckets[0]
        o = b.offsets[next(i for i, q in enumerate(b.params) if q is model.table)]
        table_ema = lambda: b.ema[o : o + rows * dim].view(rows, dim)  # noqa: E731
        five = [p.detach().clone() for p in model.parameters()] + [b.master.clone(), b.exp_avg.clone(), b.exp_avg_sq.clone(), b.ema.clone()]
        assert not torch.equal(b.ema, b.master) and torch.equal(table_ema()[idle], model.table.detach()[idle].float())
        with torch.no_grad():
            model.table[idle] += 0.5
        eng.sync_master_from_params()
        old = table_ema()[idle].clone()
        eng.begin_step()
        model(torch.randint(0, 1000, (20,), generator=g).to(dev())).backward()
        eng.step(2.5e-5)
        torch.cuda.synchronize()
        assert_ema_step(old, model.table.detach()[idle].float(), table_ema()[idle], d)
        assert float((table_ema()[idle] - old).abs().min()) > 0.4 * 0.01
        res[sparse] = five + [b.master.clone(), b.ema.clone()]
    assert all(torch.equal(x, y) for x, y in zip(res[True], res[False]))


# ------------------------------------------------------------------------------- 11. sample_actions on the averaged policy
def test_sample_actions_inside_ema_weights_is_the_policy_of_model_ema_safetensors(tmp_path):
    from kai0_amd.checkpoint import load_model_safetensors
    from kai0_amd.model import PI0Pytorch

    tr, pcfg, ocfg = _trainer(0.9)  # a short memory: after 4 steps the average is visibly not the iterate
    for step in range(4):
        tr.train_step(*_batch(ocfg, 200 + step))
    obs, _, noise, _ = _batch(ocfg, 300)
    m = tr.model
    m.eval()
    try:
        tr.params_ready()
        raw = m.sample_actions(dev(), obs, noise=noise, num_steps=10).clone()
        raw_engine = m._engine
        with tr.ema_weights():
            assert m._engine is None  # dropped on entry
            avg = m.sample_actions(dev(), obs, noise=noise, num_steps=10).clone()
            assert m._engine is not None and m._engine is not raw_engine
        assert m._engine is None  # ... and on exit
        again = m.sample_actions(dev(), obs, noise=noise, num_steps=10).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(avg).all() and not torch.equal(avg, raw)
        assert torch.equal(again, raw)  # raw weights back bit for bit, no graph captured on the averaged ones replayed
        path = tr.save_checkpoint(str(tmp_path / "ck"))
        assert sorted(os.listdir(path)) == ["metadata.pt", "model.safetensors", "model_ema.safetensors", "optimizer.pt"]
        assert torch.equal(m.sample_actions(dev(), obs, noise=noise, num_steps=10), raw)  # the writer left the raw weights behind
        fresh = PI0Pytorch(pcfg)
        load_model_safetensors(fresh, os.path.join(path, "model_ema.safetensors"))
        fresh.train_augmentation = False
        fresh = fresh.to(dev()).eval()
        for (k, p), (_, q) in zip(fresh.named_parameters(), m.named_parameters()):
            assert p.dtype == q.dtype, k
        got = fresh.sample_actions(dev(), obs, noise=noise, num_steps=10)
        torch.cuda.synchronize()
        assert torch.equal(got, avg)
        fresh_raw = PI0Pytorch(pcfg)
        load_model_safetensors(fresh_raw, os.path.join(path, "model.safetensors"))
        fresh_raw.train_augmentation = False
        assert torch.equal(fresh_raw.to(dev()).eval().sample_actions(dev(), obs, noise=noise, num_steps=10), raw)
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            with tr.ema_weights():
                tr.train_step(*_batch(ocfg, 301))
    finally:
        m.invalidate_inference_engine()
        m.train()


def test_fused_adamw_with_ema_on_the_gpu():
    """FusedAdamW(ema_decay=...): the same parameters as without, EMA within the bound every step."""
    from kai0_amd.optim import FusedAdamW

    def params():
        g = torch.Generator(device=dev()).manual_seed(1)
        return [(torch.randn(1000, 33, device=dev(), generator=g) * 0.02).to(BF16).requires_grad_(True),
                (torch.randn(513, device=dev(), generator=g) * 0.02).requires_grad_(True)]  # fmt: skip

    a, b = params(), params()
    oa = FusedAdamW(a, lr=1e-2, weight_decay=1e-2, ema_decay=0.999)
    ob = FusedAdamW(b, lr=1e-2, weight_decay=1e-2)
    g = torch.Generator(device=dev()).manual_seed(2)
    for _ in range(3):
        prev = [e.clone() for e in oa.ema_params()]
        for p, q in zip(a, b):
            p.grad = (torch.randn(p.shape, device=dev(), generator=g) * 3).to(p.dtype)
            q.grad = p.grad.clone()
        oa.step(), ob.step()
        for e0, e, ms in zip(prev, oa.ema_params(), oa.master_params()):
            assert_ema_step(e0, ms, e, 0.999)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(oa.master_params(), ob.master_params()))
