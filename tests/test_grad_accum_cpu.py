"""Gradient accumulation over micro-batches on CPU: `preprocessing.slice_observation`, `ShardedDataParallel.end_micro_batch()`,
`Trainer(micro_batch=...)`, checkpoints.

The shard arithmetic is `TorchShardOps` (tests/test_sharded_cpu.py), which has no `grad_accum`: the engine then adds the gradient
shards with torch (`acc.copy_` / `acc.add_`), the same single f32 add per element the HIP kernel `kai0_grad_accum` performs
(tests/test_grad_accum_gpu.py) — collectives, bucket bookkeeping and the Trainer are the code the GPU runs."""

import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_sharded_cpu import TorchShardOps, UnitStack, _done, _init, _spawn, _tiny_oracle_trainer, _toy_model  # noqa: E402


def _engine(model, world=1, rank=0, **kw):
    from kai0_amd.sharded import ShardedDataParallel

    base = dict(world_size=world, rank=rank, ops=TorchShardOps(), weight_decay=0.0, max_grad_norm=1.0, bucket_bytes=1500)
    if hasattr(model, "sharding_units"):
        base["units"] = model.sharding_units()
    base.update(kw)
    eng = ShardedDataParallel(list(model.named_parameters()), **base)
    if hasattr(model, "sharding_units"):
        model.hooks = eng
    return eng


def _state(eng):
    return [t.clone() for b in eng.buckets for t in (b.master, b.exp_avg, b.exp_avg_sq, b.param_shard)]


# ------------------------------------------------------------------------------------------------ slice_observation
def _obs_fields(B):
    g = torch.Generator().manual_seed(0)
    return dict(images={"base_0_rgb": torch.randn(B, 3, 4, 4, generator=g), "left_wrist_0_rgb": torch.randn(B, 3, 4, 4, generator=g)},
                image_masks={"base_0_rgb": torch.ones(B, dtype=torch.bool), "left_wrist_0_rgb": torch.arange(B) % 2 == 0},
                state=torch.randn(B, 5, generator=g), tokenized_prompt=torch.randint(0, 9, (B, 7), generator=g),
                tokenized_prompt_mask=torch.rand(B, 7, generator=g) < 0.5)  # fmt: skip


@pytest.mark.parametrize("kind", ["Observation", "SimpleObs"])
@pytest.mark.parametrize("with_progress", [False, True])
def test_slice_observation(kind, with_progress):
    from kai0_amd.preprocessing import Observation, slice_observation
    from oracle.pi0_oracle import SimpleObs

    B, lo, hi = 6, 2, 5
    f = _obs_fields(B)
    if with_progress:
        f["progress"] = torch.linspace(-1, 1, B)
    if kind == "SimpleObs":
        f.update(token_ar_mask=None, token_loss_mask=None, note="kept", scalar=torch.tensor(3.0), table=torch.arange(B + 1))
    obs = (Observation if kind == "Observation" else SimpleObs)(**f)
    cut = slice_observation(obs, lo, hi)
    assert type(cut) is type(obs) and cut is not obs
    for name in ("state", "tokenized_prompt", "tokenized_prompt_mask") + (("progress",) if with_progress else ()):
        assert torch.equal(getattr(cut, name), getattr(obs, name)[lo:hi]), name
    for name in ("images", "image_masks"):
        d = getattr(cut, name)
        assert list(d) == list(getattr(obs, name)) and d is not getattr(obs, name)
        assert all(torch.equal(d[k], getattr(obs, name)[k][lo:hi]) for k in d), name
    assert cut.token_ar_mask is None and cut.token_loss_mask is None
    if not with_progress:
        assert getattr(cut, "progress", None) is None
    if kind == "Observation":
        assert cut.image_original is None and cut.episode_index is None
    else:  # whatever is not batched passes through: strings, 0-d tensors, tensors of another leading dimension
        assert cut.note == "kept" and cut.scalar is obs.scalar and cut.table is obs.table
    assert obs.state.shape[0] == B and obs.images["base_0_rgb"].shape[0] == B  # the original is untouched
    whole = slice_observation(obs, 0, B)
    assert torch.equal(whole.state, obs.state)


# ------------------------------------------------------------------------------------------------ engine, world 1
@pytest.mark.parametrize("clip", [None, 0.05])
@pytest.mark.parametrize("ema", [None, 0.99])
def test_engine_two_micro_batches_equal_one_backward_of_the_summed_loss(clip, ema):
    """f32 parameters: autograd adds the two uses' gradients with one f32 add per element, the engine adds the two micro-batches'
    with one f32 add per element, and an f32 add is commutative — parameters, masters, moments, EMA and the norm are bit-identical."""
    data = torch.randn(4, 2, 5, 24, generator=torch.Generator().manual_seed(1))
    ma, mb = _toy_model(seed=0), _toy_model(seed=0)
    ea, eb = _engine(ma, max_grad_norm=clip, ema_decay=ema, bucket_bytes=1024), _engine(mb, max_grad_norm=clip, ema_decay=ema, bucket_bytes=1024)
    assert len(ea.buckets) > 1
    for s in range(4):
        ea.begin_step()
        (ma(data[s, 0]).pow(2).mean() / 2).backward()
        ea.end_micro_batch()
        assert ea.step_count == s and ea._micro == 1 and all(b.pending == len(b.params) and not b.arrived for b in ea.buckets)
        (ma(data[s, 1]).pow(2).mean() / 2).backward()
        na = ea.step(3e-3).clone()
        eb.begin_step()
        (mb(data[s, 0]).pow(2).mean() / 2 + mb(data[s, 1]).pow(2).mean() / 2).backward()
        nb = eb.step(3e-3).clone()
        assert ea.step_count == eb.step_count == s + 1 and ea._micro == 0
        if clip is not None:
            assert torch.equal(na, nb) and float(na) > clip  # the norm of the ACCUMULATED gradient, and it clips
    assert all(torch.equal(x, y) for x, y in zip(_state(ea), _state(eb)))
    if ema is not None:
        assert all(torch.equal(a.ema, b.ema) and not torch.equal(a.ema, a.master) for a, b in zip(ea.buckets, eb.buckets))
    assert all(b.acc.dtype == torch.float32 and b.acc.numel() == b.shard for b in ea.buckets)
    assert not any(hasattr(b, "acc") for b in eb.buckets)  # never allocated in an engine that never accumulates
    assert ea.optimizer_state_bytes() == eb.optimizer_state_bytes()
    sa, sb = ea.state_dict(), eb.state_dict()
    assert sa.keys() == sb.keys() and all(sa["state"][i].keys() == sb["state"][i].keys() for i in sa["state"])


def test_first_micro_batch_overwrites_the_accumulator():
    model = _toy_model(seed=0)
    eng = _engine(model, bucket_bytes=1024)
    x = torch.randn(2, 5, 24, generator=torch.Generator().manual_seed(2))
    model(x[0]).pow(2).mean().backward()
    eng.end_micro_batch()
    model(x[1]).pow(2).mean().backward()
    eng.step(1e-3)
    for b in eng.buckets:
        b.acc.fill_(float("nan"))  # dead between steps: whatever it holds must not reach the next one
    model(x[0]).pow(2).mean().backward()
    eng.end_micro_batch()
    assert all(torch.equal(b.acc, b.grad_shard.float()) for b in eng.buckets)
    model(x[1]).pow(2).mean().backward()
    eng.step(1e-3)
    assert all(bool(torch.isfinite(t).all()) for t in _state(eng))


def test_end_micro_batch_inside_ema_weights_raises():
    model = UnitStack(seed=3)
    eng = _engine(model, ema_decay=0.99)
    model(torch.randn(6, 16, generator=torch.Generator().manual_seed(5))).pow(2).mean().backward()
    eng.step(3e-3)
    with eng.ema_weights():
        with pytest.raises(RuntimeError, match="inside ema_weights"):
            eng.end_micro_batch()


def test_begin_step_discards_an_aborted_accumulation():
    """One micro-batch accumulated, then the step dies (an exception in the second forward): after begin_step() the next full
    (two-micro-batch) step is a fresh engine's, bit for bit."""
    data = torch.randn(3, 6, 16, generator=torch.Generator().manual_seed(5))
    res = []
    for abort in (True, False):
        model = UnitStack(seed=3)
        eng = _engine(model)
        if abort:
            eng.begin_step()
            (model(data[2]).pow(2).mean() / 2).backward()
            eng.end_micro_batch()
            assert eng._micro == 1  # ... and the step never reaches its second backward
        eng.begin_step()
        assert eng._micro == 0
        for i in range(2):
            (model(data[i]).pow(2).mean() / 2).backward()
            eng.end_micro_batch() if i == 0 else eng.step(3e-3)
        res.append(_state(eng) + [eng._norm.clone()])
    assert all(torch.equal(x, y) for x, y in zip(*res))


# ------------------------------------------------------------------------------------------------ Trainer
def _slice(obs, lo, hi):
    from kai0_amd.preprocessing import slice_observation

    return slice_observation(obs, lo, hi)


def _batch4():
    from tiny import tiny_cfgs

    from oracle.pi0_oracle import synthetic_batch

    _, ocfg = tiny_cfgs()
    return synthetic_batch(ocfg, 4, seed=0)


def test_trainer_micro_batch_must_divide_the_batch(monkeypatch):
    from kai0_amd.train import Trainer

    monkeypatch.delenv("KAI0_MICRO_BATCH", raising=False)
    tr, model, *_ = _tiny_oracle_trainer(1, 0)
    assert tr.micro_batch is None
    obs, actions, noise, time = _batch4()
    tr.micro_batch = 3
    with pytest.raises(ValueError, match="does not divide"):
        tr.train_step(obs, actions, noise, time)
    assert tr.global_step == 0 and tr.engine.step_count == 0
    monkeypatch.setenv("KAI0_MICRO_BATCH", "2")  # the default comes from the environment
    model2 = _tiny_oracle_trainer(1, 0)[1]
    assert Trainer(model2, shard_ops=TorchShardOps(), bucket_bytes=64 << 10).micro_batch == 2
    monkeypatch.setenv("KAI0_MICRO_BATCH", "0")
    model3 = _tiny_oracle_trainer(1, 0)[1]
    assert Trainer(model3, shard_ops=TorchShardOps(), bucket_bytes=64 << 10).micro_batch is None


def _worker_trainer_accum(rank, world, port, tmp, out, mode):
    _init(rank, world, port)
    torch.set_num_threads(2)
    tr, model, *_ = _tiny_oracle_trainer(world, rank, mode=mode)
    tr.micro_batch = 1
    assert tr.engine.mode == mode
    obs, actions, noise, time = _batch4()
    lo, hi = 2 * rank, 2 * rank + 2  # this rank's two samples of the global batch of four, run as 2 x 1
    losses = []
    for _ in range(3):
        losses.append(float(tr.train_step(_slice(obs, lo, hi), actions[lo:hi], noise[lo:hi], time[lo:hi])))
        if mode == "fsdp":  # the full parameter buffers are released between micro-batches and after the step
            assert all(not tr.engine.buckets[bi].resident for ids in tr.engine.groups[1:] for bi in ids)
    assert tr.global_step == 3 and tr.engine.step_count == 3
    assert all(b.acc.numel() == b.shard for b in tr.engine.buckets)
    tr.params_ready()
    torch.save({"losses": losses, "norm": float(tr.last_grad_norm), "params": {n: p.detach().float().clone() for n, p in model.named_parameters()}},
               os.path.join(out, f"w2_rank{rank}.pt"))  # fmt: skip
    _done(rank, tmp)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode", ["zero2", "fsdp"])
def test_trainer_world2_with_two_micro_batches_matches_world1_unsplit(tmp_path, mode):
    """Global batch of 4: two ranks x (2 micro-batches of 1) against one process, one backward of 4.  Tolerances: those of
    test_sharded_cpu.py::test_trainer_world2_matches_world1_and_checkpoint_resumes_at_another_world_size."""
    out = str(tmp_path)
    _spawn(_worker_trainer_accum, 2, out, mode)
    w2 = [torch.load(os.path.join(out, f"w2_rank{r}.pt"), weights_only=False) for r in range(2)]
    for n in w2[0]["params"]:
        assert torch.equal(w2[0]["params"][n], w2[1]["params"][n]), n
    tr, model, *_ = _tiny_oracle_trainer(1, 0)
    obs, actions, noise, time = _batch4()
    init = {n: p.detach().float().clone() for n, p in model.named_parameters()}
    l1 = [float(tr.train_step(obs, actions, noise, time)) for _ in range(3)]
    assert not any(hasattr(b, "acc") for b in tr.engine.buckets)
    mean_w2 = [(a + b) / 2 for a, b in zip(w2[0]["losses"], w2[1]["losses"])]
    assert all(abs(a - b) < 2e-2 * abs(b) for a, b in zip(mean_w2, l1)), (mean_w2, l1)
    assert abs(w2[0]["norm"] - float(tr.last_grad_norm)) < 5e-2 * float(tr.last_grad_norm)
    num = den = 0.0
    for n, p in model.named_parameters():
        d1, d2 = p.detach().float() - init[n], w2[0]["params"][n] - init[n]
        num += float((d1 - d2).pow(2).sum())
        den += float(d1.pow(2).sum())
    print(f"world 2 x 2 micro-batches vs world 1 unsplit ({mode}): rel-L2 of the parameter movement {(num / den) ** 0.5:.4f}")
    assert (num / den) ** 0.5 < 0.15, (num / den) ** 0.5


def test_checkpoints_of_accumulating_and_plain_trainers_are_interchangeable(tmp_path):
    """The accumulators are dead between steps: optimizer.pt has the same keys either way, a checkpoint written by an accumulating
    trainer resumes in a plain one and the reverse, and the resumed runs continue on the writer's trajectory exactly."""
    obs, actions, noise, time = _batch4()
    obs2, act2, noise2, time2 = _slice(obs, 0, 2), actions[:2], noise[:2], time[:2]

    def trainer(micro):
        tr, model, *_ = _tiny_oracle_trainer(1, 0)
        tr.micro_batch = micro
        return tr, model

    files, after = {}, {}
    for name, micro in (("accum", 1), ("plain", None)):
        tr, model = trainer(micro)
        for _ in range(2):
            tr.train_step(obs2, act2, noise2, time2)
        path = tr.save_checkpoint(str(tmp_path / name))
        assert sorted(os.listdir(path)) == ["metadata.pt", "model.safetensors", "optimizer.pt"]
        files[name] = torch.load(os.path.join(path, "optimizer.pt"), weights_only=True)
        tr.train_step(obs2, act2, noise2, time2)  # the writer's own third step
        tr.params_ready()
        after[name] = [p.detach().clone() for p in model.parameters()]
    a, p = files["accum"], files["plain"]
    assert a.keys() == p.keys() and a["param_names"] == p["param_names"] and a["state"].keys() == p["state"].keys()
    assert all(a["state"][i].keys() == p["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq", "master"} for i in a["state"])
    for src, micro in (("accum", None), ("plain", 1)):  # loaded into the OTHER kind of trainer
        tr, model = trainer(micro)
        assert tr.load_checkpoint(str(tmp_path / src)) == 2
        loss = tr.train_step(obs2, act2, noise2, time2)
        assert bool(torch.isfinite(loss)) and tr.global_step == 3
    for src, micro in (("accum", 1), ("plain", None)):  # and into its own kind: the writer's third step, bit for bit
        tr, model = trainer(micro)
        tr.load_checkpoint(str(tmp_path / src))
        tr.train_step(obs2, act2, noise2, time2)
        tr.params_ready()
        assert all(torch.equal(x, y) for x, y in zip(model.parameters(), after[src])), src
