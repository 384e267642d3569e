"""Parameter EMA of the sharded trainer on CPU: engine, partition independence, state dicts, the row-sparse path, `ema_weights()`,
the Trainer's checkpoints, `train_loop` under KAI0_EMA=1 and `create_trained_policy(..., ema=True)`.

The shard arithmetic is `TorchShardOps` (tests/test_sharded_cpu.py), which knows nothing about the EMA: the engine then runs
`adamw` followed by `ema.lerp_(master, 1 - d)`, the same update the HIP kernel `kai0_adamw_ema` fuses (tests/test_ema_gpu.py).

Bound of one EMA step (derived, not tuned).  Given f32 `e`, `p`, `d`, e' = e + (1 - d)(p - e) goes through at most four roundings
(1 - d, the difference, the product, the sum), each at most 2^-24 relative.  With M = max(|e|, |p|): |p - e| <= 2M, 1 - d <= 1 and
e' lies between e and p, so the first three contribute at most 2^-23 M each and the last 2^-24 M: 1.75 * 2^-22 M in all.  Against
the same expression in float64 from the same f32 inputs (d as f32): |e' - ref| <= 2^-21 * max(|e|, |p|) elementwise.  Over K
steps the comparison is step by step (previous EMA as stored, new master as stored), so the bound does not grow with K."""

import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_sharded_cpu import TorchRowOps, TorchShardOps, UnitStack, _done, _Embed, _init, _spawn  # noqa: E402

D = 0.99
W32 = 1.0 - float(np.float32(D))  # 1 - d as the update forms it: from the decay as an f32


def assert_ema_step(prev, master, new, d=D):
    """|new - float64(prev + (1 - d32)(master - prev))| <= 2^-21 max(|prev|, |master|), elementwise (module docstring)."""
    d32 = float(np.float32(d))
    ref = prev.double() + (1.0 - d32) * (master.double() - prev.double())
    bound = 2.0**-21 * torch.maximum(prev.abs(), master.abs()).double()
    err = (new.double() - ref).abs()
    assert bool((err <= bound).all()), (float(err.max()), float(bound.max()))


def _engine(model, world=1, rank=0, **kw):
    from kai0_amd.sharded import ShardedDataParallel

    base = dict(world_size=world, rank=rank, ops=TorchShardOps(), weight_decay=0.0, max_grad_norm=1.0, bucket_bytes=1500,
                units=model.sharding_units())  # fmt: skip
    base.update(kw)
    eng = ShardedDataParallel(list(model.named_parameters()), **base)
    model.hooks = eng
    return eng


# ------------------------------------------------------------------------------------------------ 1. engine, world 1
def test_engine_ema_follows_the_master_step_by_step():
    model = UnitStack(seed=3)
    eng = _engine(model, ema_decay=D)
    assert all(torch.equal(b.ema, b.master) and b.ema.dtype == torch.float32 for b in eng.buckets)  # initialised from the master
    assert eng.optimizer_state_bytes() == sum(4 * 4 * b.shard for b in eng.buckets)
    data = torch.randn(10, 6, 16, generator=torch.Generator().manual_seed(5))
    moved = 0.0
    for step in range(10):
        prev = [b.ema.clone() for b in eng.buckets]
        model(data[step]).pow(2).mean().backward()
        eng.step(3e-3)
        for b, e0 in zip(eng.buckets, prev):
            assert_ema_step(e0, b.master, b.ema)
            moved += float((b.ema - e0).abs().sum())
    assert moved > 0 and any(not torch.equal(b.ema, b.master) for b in eng.buckets)


def test_engine_without_a_decay_is_what_it_was():
    model = UnitStack(seed=3)
    eng = _engine(model)
    assert eng.ema_decay is None and not any(hasattr(b, "ema") for b in eng.buckets)
    assert eng.optimizer_state_bytes() == sum(3 * 4 * b.shard for b in eng.buckets)
    sd = eng.state_dict()
    assert all(set(ent) == {"step", "exp_avg", "exp_avg_sq", "master"} for ent in sd["state"].values())
    with pytest.raises(RuntimeError, match="without ema_decay"):
        with eng.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="without ema_decay"):
        eng.reset_ema()
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _engine(UnitStack(seed=3), ema_decay=bad)


# --------------------------------------------------------------------------------- 2. world 2 against world 1; 5. ema_weights
def _run_steps(model, eng, batches, world, lr=3e-3):
    """Steps the engine; after every step gathers the state (collective) and, on rank 0, advances an f32 `lerp_` EMA over the
    gathered masters.  Returns (last state dict, lerp reference) on rank 0."""
    sd = eng.state_dict()
    ref = {sd["param_names"][i]: ent["master"].clone() for i, ent in sd["state"].items()} if sd is not None else None
    for x in batches:
        (model(x).pow(2).mean() / world).backward()
        eng.step(lr)
        sd = eng.state_dict()
        if sd is not None:
            for i, ent in sd["state"].items():
                ref[sd["param_names"][i]].lerp_(ent["master"], W32)
    return sd, ref


def _by_name(sd, key):
    return {sd["param_names"][i]: ent[key] for i, ent in sd["state"].items()}


def _worker_world2(rank, world, port, tmp, mode):
    _init(rank, world, port)
    torch.set_num_threads(1)
    data = torch.randn(4, world, 3, 16, generator=torch.Generator().manual_seed(5))
    model = UnitStack(seed=3 + rank)  # construction broadcasts rank 0's weights; the EMA must start from THOSE
    eng = _engine(model, world, rank, mode=mode, ema_decay=D)
    assert eng.mode == mode and all(b.ema.numel() == b.shard for b in eng.buckets)
    sd2, ref2 = _run_steps(model, eng, [data[s, rank] for s in range(4)], world)
    # ---- ema_weights() at world 2 (every rank enters and leaves)
    eng.wait_params()
    before = [p.detach().clone() for p in model.parameters()]
    with eng.ema_weights():
        inside = {n: p.detach().clone() for n, p in model.named_parameters()}  # complete on every rank
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            eng.step(1e-3)
        out_in = model(data[0, 0])  # a forward inside the context (fsdp: releases and re-gathers from the EMA shards)
        eng.wait_params()
        for n, p in model.named_parameters():
            assert torch.equal(p, inside[n]), n
    if mode == "fsdp":  # released again as step() leaves them
        assert all(not eng.buckets[bi].resident for ids in eng.groups[1:] for bi in ids)
    eng.wait_params()
    for p, q in zip(model.parameters(), before):
        assert torch.equal(p, q)  # bit-identical to before entry
    assert not torch.equal(model(data[0, 0]), out_in)
    box = [inside]
    dist.broadcast_object_list(box, src=1)  # rank 1's view of the averaged weights is rank 0's
    assert all(torch.equal(inside[n], box[0][n]) for n in inside)
    if rank == 0:
        ema2, master2 = _by_name(sd2, "ema"), _by_name(sd2, "master")
        for n, p in model.named_parameters():
            assert torch.equal(inside[n], ema2[n].to(p.dtype)), n  # every trained parameter == ema.to(p.dtype)
            assert torch.equal(ema2[n], ref2[n]), n  # the f32 lerp_ sequence over this run's own gathered masters
        # ---- the same global batches at world 1
        m1 = UnitStack(seed=3)
        e1 = _engine(m1, ema_decay=D)
        sd1, ref1 = _run_steps(m1, e1, [data[s].reshape(-1, 16) for s in range(4)], 1)
        ema1, master1 = _by_name(sd1, "ema"), _by_name(sd1, "master")
        for n, p in m1.named_parameters():
            assert torch.equal(ema1[n], ref1[n]), n
            # as closely as test_sharded_cpu.py::_worker_units requires of the parameters (bf16 gradients are summed in bf16)
            tol = 1e-2 if p.dtype == torch.bfloat16 else 2e-3
            assert torch.allclose(master2[n], master1[n], atol=tol, rtol=tol), n
            assert torch.allclose(ema2[n], ema1[n], atol=tol, rtol=tol), n
            assert not torch.equal(ema2[n], master2[n]), n
    _done(rank, tmp)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("mode", ["zero2", "fsdp"])
def test_world2_ema_matches_world1_and_ema_weights_round_trips(mode):
    _spawn(_worker_world2, 2, mode)


def test_ema_weights_world1_round_trip_and_guards():
    model = UnitStack(seed=3)
    eng = _engine(model, ema_decay=D)
    data = torch.randn(3, 6, 16, generator=torch.Generator().manual_seed(5))
    for s in range(3):
        model(data[s]).pow(2).mean().backward()
        eng.step(3e-3)
    before = [p.detach().clone() for p in model.parameters()]
    masters = [b.master.clone() for b in eng.buckets]
    with eng.ema_weights():
        for b in eng.buckets:
            for p, o in zip(b.params, b.offsets):
                assert torch.equal(p.detach().reshape(-1), b.ema[o : o + p.numel()].to(p.dtype))
        assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), before))
        for call in (lambda: eng.step(1e-3), eng.sync_master_from_params, lambda: eng.load_state_dict({}), lambda: eng.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                call()
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    assert all(torch.equal(b.master, m) for b, m in zip(eng.buckets, masters))
    # an exception inside the context still restores the raw weights
    with pytest.raises(KeyError):
        with eng.ema_weights():
            raise KeyError("x")
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before)) and not eng._in_ema
    # restored from the bytes kept on entry, not re-rounded from the masters: weights that are NOT the rounded master survive
    with torch.no_grad():
        model.blocks[0].weight.add_(0.25)
    odd = model.blocks[0].weight.detach().clone()
    with eng.ema_weights():
        pass
    assert torch.equal(model.blocks[0].weight, odd)
    model(data[0]).pow(2).mean().backward()  # and training goes on
    eng.step(3e-3)


# ----------------------------------------------------------------------------------------- 3. state dicts across world sizes
def _snapshot(eng):
    sd = eng.state_dict()
    return None if sd is None else {k: _by_name(sd, k) for k in ("master", "exp_avg", "exp_avg_sq", "ema")}


def _worker_resume(rank, world, port, tmp):
    """Both ranks see the SAME batch and the loss carries 1/2: the summed gradient is bit for bit the world-1 gradient (halving and
    re-adding two equal halves is exact), so the world-2 run and the world-1 run are the same trajectory and can be compared exactly."""
    _init(rank, world, port)
    torch.set_num_threads(1)
    data = torch.randn(5, 6, 16, generator=torch.Generator().manual_seed(9))
    model = UnitStack(seed=3)
    eng = _engine(model, world, rank, mode="fsdp", ema_decay=D)
    for s in range(3):
        (model(data[s]).pow(2).mean() / world).backward()
        eng.step(3e-3)
    sd = eng.state_dict([n for n, _ in model.named_parameters()])
    eng.wait_params()
    if rank == 0:
        assert all(set(ent) == {"step", "exp_avg", "exp_avg_sq", "master", "ema"} for ent in sd["state"].values())
        full_m = UnitStack(seed=3)  # the uninterrupted run, world 1, 5 steps
        full_e = _engine(full_m, ema_decay=D)
        for s in range(5):
            full_m(data[s]).pow(2).mean().backward()
            full_e.step(3e-3)
        want = _snapshot(full_e)

        def resumed(state):
            m = UnitStack(seed=77)  # other initial weights: everything must come from the checkpoint
            m.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
            e = _engine(m, ema_decay=D)
            e.load_state_dict(state)
            return m, e

        m1, e1 = resumed(sd)
        assert e1.step_count == 3
        for s in range(3, 5):
            m1(data[s]).pow(2).mean().backward()
            e1.step(3e-3)
        got = _snapshot(e1)
        for k in want:
            for n in want[k]:
                assert torch.equal(got[k][n], want[k][n]), (k, n)
        for p, q in zip(m1.parameters(), full_m.parameters()):
            assert torch.equal(p, q)
        # a state without "ema" (every checkpoint written before; the reference's optimizer.pt): EMA == master
        for ent in sd["state"].values():
            del ent["ema"]
        _, e2 = resumed(sd)
        assert all(torch.equal(b.ema, b.master) for b in e2.buckets)
        assert any(float(b.master.abs().sum()) > 0 for b in e2.buckets)
        # ... also where the master itself comes from the parameters (torch-shaped entries without `master`)
        for ent in sd["state"].values():
            del ent["master"]
        m3, e3 = resumed(sd)
        assert all(torch.equal(b.ema, b.master) for b in e3.buckets)
        b, o = e3._where[m3.head.weight]
        assert torch.equal(b.ema[o : o + m3.head.weight.numel()].view_as(m3.head.weight), m3.head.weight.detach().float())
    _done(rank, tmp)


@pytest.mark.timeout(180)
def test_state_dict_from_world2_resumes_at_world1_bit_identically():
    _spawn(_worker_resume, 2)


# ------------------------------------------------------------------------------------------------ 4. row-sparse path
class TorchRowEmaOps(TorchRowOps):
    """+ kai0_adamw_rows_ema in torch: an idle row (no gradient, flag clear) is skipped, EMA included."""

    ema_calls = 0

    def adamw_rows_ema(self, master, m, v, ema, grad, param, row_len, row_active, *, ema_decay, **kw):
        TorchRowEmaOps.ema_calls += 1
        rows = master.numel() // row_len
        nz = (grad.view(rows, row_len).float() != 0).any(1)
        row_active |= nz.to(torch.uint8)
        w = 1.0 - float(np.float32(ema_decay))
        for r in torch.nonzero(row_active).flatten().tolist():
            sl = slice(r * row_len, (r + 1) * row_len)
            self.adamw(master[sl], m[sl], v[sl], grad[sl], param[sl], **kw)
            ema[sl].lerp_(master[sl], w)


def test_row_sparse_update_with_ema_equals_the_dense_one_and_sees_rewritten_idle_rows():
    from kai0_amd.sharded import ShardedDataParallel

    rows, dim = 1500, 72
    idle = torch.tensor([1210, 1300, 1499])  # never drawn below
    res = {}
    for sparse in (True, False):
        model = _Embed(rows, dim, seed=3)
        model.table._kai0_grad_accumulates = True
        eng = ShardedDataParallel(list(model.named_parameters()), world_size=1, rank=0, ops=TorchRowEmaOps(), weight_decay=1e-10,
                                  bucket_bytes=1 << 30, ema_decay=D)  # fmt: skip
        eng._sparse_rows = sparse
        TorchRowEmaOps.ema_calls = 0
        g = torch.Generator().manual_seed(100)
        for step in range(6):
            eng.begin_step()
            model(torch.randint(0, 1000, (20 + 5 * step,), generator=g)).backward()
            eng.step(2.5e-5)
        b = eng.buckets[0]
        o = b.offsets[next(i for i, q in enumerate(b.params) if q is model.table)]
        table_ema = lambda: b.ema[o : o + rows * dim].view(rows, dim)  # noqa: E731
        if sparse:
            (first, nrows, rl, active), = eng._sparse_segments(b)
            assert TorchRowEmaOps.ema_calls == 6 and 0 < int(active.sum()) < nrows and not bool(active[idle - (first - o) // dim].any())
        else:
            assert TorchRowEmaOps.ema_calls == 0
        six = ([p.detach().clone() for p in model.parameters()], b.master.clone(), b.exp_avg.clone(), b.exp_avg_sq.clone(), b.ema.clone())
        assert not torch.equal(b.ema, b.master) and torch.equal(table_ema()[idle], model.table.detach()[idle].float())
        # weights written into idle rows after construction (model_arithmetic): their EMA must start moving towards them
        with torch.no_grad():
            model.table[idle] += 0.5
        eng.sync_master_from_params()
        old = table_ema()[idle].clone()
        eng.begin_step()
        model(torch.randint(0, 1000, (20,), generator=g)).backward()
        eng.step(2.5e-5)
        new_master = model.table.detach()[idle].float()
        assert torch.equal(table_ema()[idle], old.clone().lerp_(new_master, W32))  # moved by (1 - d) of the jump
        assert float((table_ema()[idle] - old).abs().min()) > 0.4 * W32
        res[sparse] = (*six, b.master.clone(), b.ema.clone())
    for x, y in zip(res[True], res[False]):
        if isinstance(x, list):
            assert all(torch.equal(a, c) for a, c in zip(x, y))
        else:
            assert torch.equal(x, y)


def test_reset_ema_restarts_the_average_from_the_master():
    model = UnitStack(seed=3)
    eng = _engine(model, ema_decay=D)
    data = torch.randn(2, 6, 16, generator=torch.Generator().manual_seed(5))
    for s in range(2):
        model(data[s]).pow(2).mean().backward()
        eng.step(3e-3)
    ema = [b.ema.clone() for b in eng.buckets]
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5)
    eng.sync_master_from_params()  # documented: leaves the EMA alone
    assert all(torch.equal(b.ema, e) for b, e in zip(eng.buckets, ema))
    eng.reset_ema()
    assert all(torch.equal(b.ema, b.master) for b in eng.buckets)


# ------------------------------------------------------------------------------------- 6. Trainer, train_loop, policy
def _loop_helpers():
    import test_train_loop_cpu as tl

    return tl


def _load(path):
    from safetensors.torch import load_file

    return load_file(str(path))


@pytest.mark.timeout(600)
def test_train_loop_writes_and_resumes_the_ema_only_under_KAI0_EMA(tmp_path, monkeypatch):
    tl = _loop_helpers()
    monkeypatch.delenv("KAI0_EMA", raising=False)
    lines = []
    from kai0_amd.train import train_loop

    def run(cfg, seed=0):
        _, ocfg = tl._cfgs()
        return train_loop(cfg, device="cpu", shard_ops=TorchShardOps(), model=tl._stand_in(ocfg, seed), log=lines.append)

    plain = run(tl._config(tmp_path, exp_name="plain", overwrite=True, num_train_steps=4))
    ck = tmp_path / "ckpt" / "tiny_loop"
    assert sorted(os.listdir(ck / "plain" / "4")) == ["metadata.pt", "model.safetensors", "optimizer.pt"]  # exactly today's entries
    assert sum("EMA off" in l for l in lines) == 1 and not any("EMA on" in l for l in lines)
    opt = torch.load(ck / "plain" / "4" / "optimizer.pt", weights_only=True)
    assert all("ema" not in ent for ent in opt["state"].values())

    monkeypatch.setenv("KAI0_EMA", "1")
    del lines[:]
    full = run(tl._config(tmp_path, exp_name="full", overwrite=True))
    assert sum("EMA on: decay=0.99" in l for l in lines) == 1
    assert [r["loss"] for r in full[:4]] == [r["loss"] for r in plain]  # the EMA does not perturb training
    assert sorted(os.listdir(ck / "full" / "6")) == ["metadata.pt", "model.safetensors", "model_ema.safetensors", "optimizer.pt"]
    raw, ema = _load(ck / "full" / "6" / "model.safetensors"), _load(ck / "full" / "6" / "model_ema.safetensors")
    assert list(raw) == list(ema) and all(raw[k].dtype == ema[k].dtype and raw[k].shape == ema[k].shape for k in raw)
    assert sum(not torch.equal(raw[k], ema[k]) for k in raw) > len(raw) // 2
    opt = torch.load(ck / "full" / "6" / "optimizer.pt", weights_only=True)
    names = opt["param_names"]
    from safetensors import safe_open

    with safe_open(str(ck / "full" / "6" / "model_ema.safetensors"), "pt") as f, safe_open(str(ck / "full" / "6" / "model.safetensors"), "pt") as g:
        alias = {k: v for k, v in f.metadata().items() if k != "format"}  # tied weights: dropped name -> kept name
        assert f.metadata() == g.metadata() and alias  # the same tied lm_head handling
    for i, ent in opt["state"].items():  # the file is the f32 EMA of optimizer.pt rounded to the parameter's dtype
        k = alias.get(names[i], names[i])
        assert ent["ema"].dtype == torch.float32 and torch.equal(ema[k], ent["ema"].to(ema[k].dtype)), names[i]
    dead = [k for k in raw if k not in {alias.get(names[i], names[i]) for i in opt["state"]}]
    assert all(torch.equal(raw[k], ema[k]) for k in dead)  # untrained parameters keep their value in both files
    # cut after 4 steps, resume to 6: the average continues exactly
    run(tl._config(tmp_path, exp_name="cut", num_train_steps=4, overwrite=True))
    run(tl._config(tmp_path, exp_name="cut", resume=True), seed=123)
    ema_r = _load(ck / "cut" / "6" / "model_ema.safetensors")
    opt_r = torch.load(ck / "cut" / "6" / "optimizer.pt", weights_only=True)
    assert all(torch.equal(ema[k], ema_r[k]) for k in ema)
    assert all(torch.equal(opt["state"][i]["ema"], opt_r["state"][i]["ema"]) for i in opt["state"])
    # config.ema_decay = None under KAI0_EMA=1 still means off
    del lines[:]
    run(tl._config(tmp_path, exp_name="none", overwrite=True, num_train_steps=2, ema_decay=None))
    assert sorted(os.listdir(ck / "none" / "2")) == ["metadata.pt", "model.safetensors", "optimizer.pt"]
    assert sum("EMA off" in l for l in lines) == 1


def test_trainer_checkpoint_with_ema_and_the_policy_that_serves_it(tmp_path):
    from kai0_amd import normalize, policy
    from kai0_amd import training_config as tc
    from kai0_amd.train import Trainer

    tl = _loop_helpers()
    G = np.load(os.path.join(HERE, "golden", "host_pipeline.npz"))
    pcfg, ocfg = tl._cfgs()
    pcfg, ocfg = dataclasses.replace(pcfg, max_token_len=64), dataclasses.replace(ocfg, max_token_len=64)
    cfg = tc.TrainConfig(name="tiny_agilex", exp_name="t", model=pcfg, checkpoint_base_dir=str(tmp_path / "ckpt"),
                         data=tc.LerobotAgilexDataConfig(repo_id="tiny_agilex", default_prompt="Flatten and fold the cloth.",
                                                         tokenizer_model=G["tok.model"].tobytes(), use_delta_joint_actions=False))  # fmt: skip
    rng = np.random.default_rng(0)
    q = np.sort(rng.normal(size=(2, 32)), axis=0)
    stats = {k: normalize.NormStats(mean=rng.normal(size=32), std=rng.uniform(0.5, 2, 32), q01=q[0] - 1.5, q99=q[1] + 1.5)
             for k in ("state", "actions")}  # fmt: skip
    data_config = dataclasses.replace(cfg.data.create(tmp_path / "assets", cfg.model), norm_stats=stats)
    tr = Trainer(tl._stand_in(ocfg), shard_ops=TorchShardOps(), bucket_bytes=64 << 10, ema_decay=0.99)
    assert tr.ema_decay == 0.99
    with torch.no_grad():  # an average that differs from the weights without running steps
        for b in tr.engine.buckets:
            b.ema.mul_(1.5)
    before = {k: v.clone() for k, v in tr.model.state_dict().items()}
    path = tr.save_checkpoint(str(cfg.checkpoint_dir), data_config=data_config, config=cfg)
    assert all(torch.equal(v, before[k]) for k, v in tr.model.state_dict().items())  # the model holds the raw weights again
    assert sorted(os.listdir(path)) == ["assets", "metadata.pt", "model.safetensors", "model_ema.safetensors", "optimizer.pt"]
    raw, ema = _load(os.path.join(path, "model.safetensors")), _load(os.path.join(path, "model_ema.safetensors"))
    assert list(raw) == list(ema) and all(raw[k].dtype == ema[k].dtype for k in raw)
    pol_raw = policy.create_trained_policy(cfg, path, pytorch_device="cpu")
    pol_ema = policy.create_trained_policy(cfg, path, pytorch_device="cpu", ema=True)
    sd_raw, sd_ema = pol_raw._model.state_dict(), pol_ema._model.state_dict()
    k = "action_out_proj.weight"  # a head outside paligemma_with_expert: loaded as stored
    assert torch.equal(sd_raw[k], raw[k]) and torch.equal(sd_ema[k], ema[k]) and not torch.equal(sd_ema[k], sd_raw[k])
    assert torch.equal(ema[k], (before[k].float() * 1.5).to(before[k].dtype))
    # resume: the engine's EMA comes back from optimizer.pt; the model from model.safetensors (raw)
    tr2 = Trainer(tl._stand_in(ocfg, seed=5), shard_ops=TorchShardOps(), bucket_bytes=64 << 10, ema_decay=0.99)
    tr2.load_checkpoint(str(cfg.checkpoint_dir))
    assert all(torch.equal(a.ema, b.ema) and torch.equal(a.master, b.master) for a, b in zip(tr.engine.buckets, tr2.engine.buckets))
    assert all(torch.equal(v, before[k]) for k, v in tr2.model.state_dict().items())
    # a checkpoint written without a decay: today's entries, and ema=True names the missing file
    tr3 = Trainer(tl._stand_in(ocfg), shard_ops=TorchShardOps(), bucket_bytes=64 << 10)
    path3 = tr3.save_checkpoint(str(tmp_path / "plain"), data_config=data_config, config=cfg)
    assert sorted(os.listdir(path3)) == ["assets", "metadata.pt", "model.safetensors", "optimizer.pt"]
    with pytest.raises(FileNotFoundError, match="model_ema.safetensors"):
        policy.create_trained_policy(cfg, path3, pytorch_device="cpu", ema=True)
    with pytest.raises(RuntimeError, match="without ema_decay"):
        with tr3.ema_weights():
            pass


def test_trainer_ema_weights_invalidates_the_inference_engine_on_both_edges():
    from kai0_amd.train import Trainer

    tl = _loop_helpers()
    _, ocfg = tl._cfgs()
    model = tl._stand_in(ocfg)
    calls = []
    model._engine = object()
    model.invalidate_inference_engine = lambda: calls.append(1)
    tr = Trainer(model, shard_ops=TorchShardOps(), bucket_bytes=64 << 10, ema_decay=0.5)
    with tr.ema_weights() as inside:
        assert inside is tr and len(calls) == 1
    assert len(calls) == 2


# ------------------------------------------------------------------------------------------------ 7. FusedAdamW
def test_fused_adamw_ema_state_dict_round_trip():
    from kai0_amd.optim import FusedAdamW

    def params():
        torch.manual_seed(0)
        return [torch.nn.Parameter(torch.randn(5, 3).to(torch.bfloat16)), torch.nn.Parameter(torch.randn(7))]

    opt = FusedAdamW(params(), ema_decay=0.999)
    assert opt.ema_decay == 0.999
    for st, e, m in zip(opt.state.values(), opt.ema_params(), opt.master_params()):
        assert set(st) == {"master", "exp_avg", "exp_avg_sq", "ema"} and e is st["ema"] and e.dtype == torch.float32
        assert torch.equal(e, m) and e.data_ptr() != m.data_ptr()
    for e in opt.ema_params():
        e.add_(1.0)
    sd = opt.state_dict()
    assert all(set(st) == {"master", "exp_avg", "exp_avg_sq", "ema"} for st in sd["state"])
    other = FusedAdamW(params(), ema_decay=0.999)
    other.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(other.ema_params(), opt.ema_params()))
    plain = FusedAdamW(params())
    assert plain.ema_decay is None and all(set(st) == {"master", "exp_avg", "exp_avg_sq"} for st in plain.state_dict()["state"])
    with pytest.raises(RuntimeError, match="without ema_decay"):
        plain.ema_params()
    other.load_state_dict(plain.state_dict())  # a state without EMA: EMA := master
    assert all(torch.equal(a, b) for a, b in zip(other.ema_params(), other.master_params()))
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdamW(params(), ema_decay=1.0)
