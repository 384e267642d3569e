"""Skipping optimizer steps whose gradient norm is not finite (`skip_nonfinite`, KAI0_SKIP_NONFINITE=1) on CPU: the engine at world 1,
two gloo ranks in both shard modes, `train_loop` with a NaN in the data, the default (off) pinned, misuse.

The shard arithmetic is `GuardedTorchOps`: tests/test_sharded_cpu.py's torch restatement plus what the HIP side gained —
`clip_coef_guard` (kai0_clip_coef_guard: a non-finite norm writes the negative coefficient and counts the step) and an `adamw` that
returns at once on a negative coefficient (AdamwEmaK::finish).  It has no fused EMA form, so the engine's second-pass EMA is what
runs here, with its own on-device test of the coefficient.  The kernels themselves: tests/test_nonfinite_guard_gpu.py.

Everything is compared bit for bit (`torch.equal`): a skipped step must leave every buffer's bytes alone."""

import os
import sys

import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_sharded_cpu import TorchShardOps, UnitStack, _done, _init, _spawn  # noqa: E402

INF, NAN = float("inf"), float("nan")


class GuardedTorchOps(TorchShardOps):
    def clip_coef_guard(self, sumsq, max_norm, coef, norm, skipped):
        norm.copy_(sumsq.sqrt())
        if not bool(torch.isfinite(norm).all()):
            from kai0_amd.optim import COEF_SKIP

            coef.fill_(COEF_SKIP)
            skipped += 1
        elif max_norm > 0:
            coef.copy_(torch.clamp(max_norm / (norm + 1e-6), max=1.0))
        else:
            coef.fill_(1.0)

    def adamw(self, master, m, v, grad, param, *, clip_coef, **kw):
        if clip_coef is not None and float(clip_coef) < 0:
            return
        super().adamw(master, m, v, grad, param, clip_coef=clip_coef, **kw)


def _engine(model, world=1, rank=0, **kw):
    from kai0_amd.sharded import ShardedDataParallel

    base = dict(world_size=world, rank=rank, ops=GuardedTorchOps(), weight_decay=0.0, max_grad_norm=1.0, bucket_bytes=1500,
                units=model.sharding_units(), skip_nonfinite=True)  # fmt: skip
    base.update(kw)
    eng = ShardedDataParallel(list(model.named_parameters()), **base)
    model.hooks = eng
    return eng


def _shards(eng):
    """Every persistent buffer of this rank: masters, moments, EMA (if any), the model copy's shard."""
    keys = ("master", "exp_avg", "exp_avg_sq", "param_shard") + (("ema",) if eng.ema_decay is not None else ())
    return [getattr(b, k).clone() for b in eng.buckets for k in keys]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ engine, world 1
@pytest.mark.parametrize("variant", ["clip", "no_clip", "ema", "micro"])
@pytest.mark.parametrize("poison", [INF, NAN])
def test_engine_skips_the_poisoned_step_and_nothing_else(poison, variant):
    """Three steps, +inf / NaN written into one gradient element of the second: state after it == state after the first, counter 1,
    step_count 3 after the third; with clipping, without (max_grad_norm=None: the norm is computed all the same), with an EMA, and
    as two micro-batches of which only the first is poisoned (the NaN sits in the f32 accumulator when the step is taken)."""
    kw = {"clip": {}, "no_clip": dict(max_grad_norm=None), "ema": dict(ema_decay=0.5), "micro": {}}[variant]
    model = UnitStack(seed=3)
    eng = _engine(model, **kw)
    assert eng.skip_nonfinite and eng.skipped_steps.dtype == torch.int32 and int(eng.skipped_steps) == 0
    data = torch.randn(3, 2, 6, 16, generator=torch.Generator().manual_seed(5))
    states, norms = [], []
    for step in range(3):
        bad = step == 1
        if variant == "micro":
            (model(data[step, 0]).pow(2).mean() / 2).backward()
            if bad:
                eng.buckets[1].flat_grad[5] = poison
            eng.end_micro_batch()
            (model(data[step, 1]).pow(2).mean() / 2).backward()
        else:
            model(data[step].reshape(-1, 16)).pow(2).mean().backward()
            if bad:
                eng.buckets[1].flat_grad[5] = poison
        norms.append(float(eng.step(3e-3)))
        eng.wait_params()
        states.append((_shards(eng), [p.detach().clone() for p in model.parameters()]))
    assert _same(states[1][0], states[0][0]) and _same(states[1][1], states[0][1])
    assert not torch.isfinite(torch.tensor(norms[1])) and all(torch.isfinite(torch.tensor(n)) for n in (norms[0], norms[2]))
    assert int(eng.skipped_steps) == 1 and eng.step_count == 3
    assert all(bool(torch.isfinite(t).all()) for t in states[2][0])
    assert not any(torch.equal(b.master, m0) for b, m0 in zip(eng.buckets, states[1][0][:: 5 if variant == "ema" else 4]))  # and training goes on
    # the counter travels with the optimizer state; a state written without it means 0
    sd = eng.state_dict()
    assert sd["skipped_steps"] == 1
    other = _engine(UnitStack(seed=3), **kw)
    other.load_state_dict(sd)
    assert int(other.skipped_steps) == 1 and other.step_count == 3
    del sd["skipped_steps"]
    other.load_state_dict(sd)
    assert int(other.skipped_steps) == 0


def test_engine_without_the_switch_is_what_it_was():
    from kai0_amd.sharded import ShardedDataParallel

    model = UnitStack(seed=3)
    eng = ShardedDataParallel(list(model.named_parameters()), world_size=1, rank=0, ops=TorchShardOps(), weight_decay=0.0)
    assert not eng.skip_nonfinite and not hasattr(eng, "skipped_steps") and "skipped_steps" not in eng.state_dict()


# ------------------------------------------------------------------------------------------------ gloo, world 2
def _worker_world2(rank, world, port, tmp, mode):
    _init(rank, world, port)
    torch.set_num_threads(1)
    data = torch.randn(3, world, 3, 16, generator=torch.Generator().manual_seed(5))
    data[1, 1, 2, 7] = NAN  # the second step's batch of rank 1 ONLY
    model = UnitStack(seed=3)
    eng = _engine(model, world, rank, mode=mode, ema_decay=0.5)
    assert eng.mode == mode

    def step(m, e, s):
        (m(data[s, rank]).pow(2).mean() / world).backward()
        norm = float(e.step(3e-3))
        e.wait_params()
        out = _shards(e), [p.detach().clone() for p in m.parameters()]
        if mode == "fsdp":
            e.release_params()
            e._issue_gather(0)
        return norm, out

    n1, after1 = step(model, eng, 0)
    box = [eng.state_dict()]  # (collective; rank 0 gets it)
    dist.broadcast_object_list(box, src=0)
    sd1 = box[0]
    n2, after2 = step(model, eng, 1)
    # rank 0's own gradient was finite: it skips because the all-reduced sum is the same NaN everywhere
    assert n1 == n1 and n2 != n2 and int(eng.skipped_steps) == 1
    assert _same(after2[0], after1[0]) and _same(after2[1], after1[1])
    n3, after3 = step(model, eng, 2)
    assert n3 == n3 and int(eng.skipped_steps) == 1 and eng.step_count == 3
    # the step after the skip == the step of a fresh engine that loaded the pre-poison state, its step counter advanced by one
    fresh_m = UnitStack(seed=77)
    fresh_m.load_state_dict({k: v.clone() for k, v in zip(model.state_dict(), after1[1])})
    fresh = _engine(fresh_m, world, rank, mode=mode, ema_decay=0.5)
    fresh.load_state_dict(sd1)
    assert fresh.step_count == 1 and int(fresh.skipped_steps) == 0
    fresh.step_count += 1
    if mode == "fsdp":
        fresh.release_params()
        fresh._issue_gather(0)
    f3, fresh3 = step(fresh_m, fresh, 2)
    assert f3 == n3 and _same(fresh3[0], after3[0]) and _same(fresh3[1], after3[1])
    assert not _same(after3[0], after2[0])
    _done(rank, tmp)


@pytest.mark.timeout(180)
@pytest.mark.parametrize("mode", ["zero2", "fsdp"])
def test_world2_poison_on_one_rank_is_skipped_by_both(mode):
    _spawn(_worker_world2, 2, mode)


# ------------------------------------------------------------------------------------------------ train_loop
def _poison_dataset(monkeypatch, bad_index):
    """FakeDataset whose sample `bad_index` carries one NaN action; returns the list the loaded indices are appended to."""
    from kai0_amd.data_loader import FakeDataset

    plain = FakeDataset.__getitem__
    seen = []

    def getitem(self, index):
        item = plain(self, index)
        seen.append(int(index))
        if int(index) == bad_index:
            item["actions"][0, 0] = NAN
        return item

    monkeypatch.setattr(FakeDataset, "__getitem__", getitem)
    return seen


def _final_weights(ck, exp, step):
    from safetensors.torch import load_file

    return load_file(str(ck / exp / str(step) / "model.safetensors"))


@pytest.mark.timeout(600)
def test_train_loop_survives_a_nan_in_the_data_only_under_KAI0_SKIP_NONFINITE(tmp_path, monkeypatch):
    import test_train_loop_cpu as tl

    from kai0_amd.train import train_loop

    lines = []

    def run(cfg, seed=0):
        _, ocfg = tl._cfgs()
        return train_loop(cfg, device="cpu", shard_ops=GuardedTorchOps(), model=tl._stand_in(ocfg, seed), log=lines.append)

    # which sample opens the batch of step 2: a recording pass over the (seeded) loader, no model
    from kai0_amd.lerobot_dataset import create_data_loader

    seen = _poison_dataset(monkeypatch, None)
    cfg0 = tl._config(tmp_path)
    it = iter(create_data_loader(cfg0, shuffle=True, skip_norm_stats=cfg0.skip_norm_stats))
    for _ in range(3):
        next(it)
    bad = seen[4]
    assert seen.count(bad) == 1
    _poison_dataset(monkeypatch, bad)
    ck = tmp_path / "ckpt" / "tiny_loop"

    # ---- switch off (today's behaviour, pinned): the NaN reaches every parameter
    monkeypatch.delenv("KAI0_SKIP_NONFINITE", raising=False)
    off = run(tl._config(tmp_path, exp_name="off", overwrite=True, num_train_steps=3))
    assert sum("non-finite guard off" in l for l in lines) == 1 and not any("non-finite guard on" in l for l in lines)
    assert "skipped" not in off[0] and off[2]["loss"] != off[2]["loss"]
    w = _final_weights(ck, "off", 3)
    assert sum(not bool(torch.isfinite(t.float()).all()) for t in w.values()) > len(w) // 2
    assert "skipped_total" not in torch.load(ck / "off" / "3" / "metadata.pt", weights_only=True)

    # ---- switch on: intervals [0], [1, 2, 3], [4, 5, 6]; step 2 is skipped, its interval's means are over steps 1 and 3
    monkeypatch.setenv("KAI0_SKIP_NONFINITE", "1")
    del lines[:]
    on = run(tl._config(tmp_path, exp_name="on", overwrite=True, num_train_steps=7, log_interval=3))
    assert sum("non-finite guard on" in l for l in lines) == 1
    assert [r["step"] for r in on] == [0, 3, 6]
    assert [r["skipped"] for r in on] == [0, 1, 0] and [r["skipped_total"] for r in on] == [0, 1, 1]
    assert all(torch.isfinite(torch.tensor([r["loss"], r["grad_norm"], r["learning_rate"]])).all() for r in on)
    assert on[0]["loss"] == off[0]["loss"]  # the guard does not perturb a clean step
    warned = [l for l in lines if "skipped=1 of 3 steps" in l]
    assert len(warned) == 1 and "skipped_total=1" in warned[0] and "step=3 " in warned[0]
    w = _final_weights(ck, "on", 7)
    assert all(bool(torch.isfinite(t.float()).all()) for t in w.values())
    meta = torch.load(ck / "on" / "7" / "metadata.pt", weights_only=True)
    assert meta["skipped_total"] == 1 and torch.load(ck / "on" / "7" / "optimizer.pt", weights_only=True)["skipped_steps"] == 1

    # ---- cut after 4 steps (the skip is behind it), resumed to 7: the count comes back, the weights are the uninterrupted run's
    run(tl._config(tmp_path, exp_name="cut", overwrite=True, num_train_steps=4, log_interval=3))
    del lines[:]
    rest = run(tl._config(tmp_path, exp_name="cut", resume=True, num_train_steps=7, log_interval=3), seed=123)
    assert sum("1 skipped so far" in l for l in lines) == 1
    assert [r["step"] for r in rest] == [6] and rest[0]["skipped"] == 0 and rest[0]["skipped_total"] == 1
    assert rest[0]["loss"] == on[2]["loss"]
    w2 = _final_weights(ck, "cut", 7)
    assert all(torch.equal(w[k], w2[k]) for k in w)


# ------------------------------------------------------------------------------------------------ misuse
def test_the_switch_needs_ops_that_know_the_guard_and_a_well_formed_value(tmp_path, monkeypatch):
    import test_train_loop_cpu as tl

    from kai0_amd.sharded import ShardedDataParallel
    from kai0_amd.train import Trainer, train_loop

    model = UnitStack(seed=3)
    with pytest.raises(TypeError, match="clip_coef_guard"):
        ShardedDataParallel(list(model.named_parameters()), world_size=1, rank=0, ops=TorchShardOps(), skip_nonfinite=True)
    _, ocfg = tl._cfgs()
    with pytest.raises(TypeError, match="clip_coef_guard"):
        Trainer(tl._stand_in(ocfg), shard_ops=TorchShardOps(), bucket_bytes=64 << 10, skip_nonfinite=True)
    tr = Trainer(tl._stand_in(ocfg), shard_ops=GuardedTorchOps(), bucket_bytes=64 << 10, skip_nonfinite=True)
    assert tr.skip_nonfinite and tr.skipped_total() == 0
    for bad in ("yes", "true", "2", ""):
        monkeypatch.setenv("KAI0_SKIP_NONFINITE", bad)
        with pytest.raises(ValueError, match="KAI0_SKIP_NONFINITE"):
            train_loop(tl._config(tmp_path), device="cpu", shard_ops=GuardedTorchOps(), model=None)
