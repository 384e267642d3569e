"""pi0 (`pi05=False`) on the GPU: the tiny HIP model against tests/golden/reference_pi0.safetensors (what the reference's own code
computes, make_reference_pi0_golden.py) at the bounds of tests/test_model_gpu.py, the inference engine's invariants, the state-token
mask-codes kernel, the `debug` training loop and a served request."""

import copy
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch
from safetensors import safe_open
from safetensors.torch import load_file

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FIX = os.path.join(HERE, "golden", "reference_pi0.safetensors")


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


@pytest.fixture(scope="module")
def pair():
    """the tiny pi0 HIP model with the fixture's weights + the fixture's batch"""
    import pi0_restatement as R
    from tiny import obs_to, tiny_cfgs

    from kai0_amd.model import PI0Pytorch
    from oracle.pi0_oracle import synthetic_batch

    with safe_open(FIX, "pt") as f:
        meta = json.loads(f.metadata()["json"])
    E = load_file(FIX)
    pcfg, ocfg05 = tiny_cfgs()
    restated = R.build_restated(ocfg05, {k[2:]: v for k, v in E.items() if k.startswith("w.")}, float(meta["std"]))
    dev = torch.device("cuda:0")
    model = PI0Pytorch(dataclasses.replace(pcfg, pi05=False, discrete_state_input=None))
    model.load_state_dict(restated.state_dict(), strict=True)
    model.train_augmentation = False
    model = model.to(dev)
    obs, actions, noise, time = synthetic_batch(restated.config, 2, seed=0)
    assert torch.equal(noise, E["noise"]) and torch.equal(time, E["time"])
    return dict(model=model, E=E, meta=meta, obs=obs, gobs=obs_to(obs, dev), actions=actions, noise=noise, time=time, dev=dev)


def _loss(pair):
    m, dev = pair["model"], pair["dev"]
    return m(pair["gobs"], pair["actions"].to(dev), noise=pair["noise"].to(dev), time=pair["time"].to(dev))


def _chunk(pair, gobs=None):
    m, dev = pair["model"], pair["dev"]
    return m.sample_actions(dev, gobs if gobs is not None else pair["gobs"], noise=pair["noise"].to(dev), num_steps=10)


def test_pi0_suffix_embedding_against_reference(pair):
    """embed_suffix: 1 state token + H action-time tokens, att [1, 1, 0, ...], no adaRMS cond; f32 heads against the reference's f32
    torch Linears (exact-f32 GEMM, other summation order: 1e-5 relative)."""
    m, dev, E = pair["model"], pair["dev"], pair["E"]
    t = pair["time"][:, None, None]
    x_t = (t * pair["noise"] + (1 - t) * pair["actions"]).to(dev)
    with torch.no_grad():
        suf, pad, att, cond = m.embed_suffix(pair["gobs"].state, x_t, pair["time"].to(dev))
    assert cond is None and suf.shape == (2, 11, 64) and suf.dtype == torch.float32
    assert torch.equal(pad.cpu(), E["suffix_pad"]) and torch.equal(att.cpu().float(), E["suffix_att"])
    r = rel(suf, E["suffix"])
    print(f"suffix embedding rel-L2 {r:.3e}")
    assert r <= 1e-5


def test_pi0_loss_and_chunk_against_reference_executed(pair):
    E = pair["E"]
    loss = _loss(pair).detach()
    assert loss.shape == (2, 10, 32) and loss.dtype == torch.float32
    out = _chunk(pair)
    assert out.shape == (2, 10, 32) and out.dtype == torch.float32
    rl, rc, mx = rel(loss, E["loss"]), rel(out, E["actions"]), float((out.float().cpu() - E["actions"]).abs().max())
    print(f"pi0 vs reference: loss rel-L2 {rl:.3e} | chunk rel-L2 {rc:.3e} max|d| {mx:.3e} (fixture floor: loss "
          f"{float(pair['meta']['floor_loss_rel_l2']):.3e}, chunk {float(pair['meta']['floor_chunk_rel_l2']):.3e})")
    assert rl <= 1e-2
    assert rc <= 3e-3 and mx <= 2e-2


def test_pi0_gradients_against_reference_executed_backward(pair):
    m, E = pair["model"], pair["E"]
    m.zero_grad(set_to_none=True)
    _loss(pair).mean().backward()
    params = dict(m.named_parameters())
    worst = 0.0
    for k in [k[5:] for k in E if k.startswith("grad.")]:
        assert params[k].grad is not None, k
        r = rel(params[k].grad, E["grad." + k])
        print(f"{r:.3e}  {k}")
        worst = max(worst, r)
        assert r <= 5e-2, (k, r)
    # parameters the reference gives no gradient get none (lm_heads, the prefix's final norm, the last prefix layer's dead half)
    no_grad = pair["meta"]["no_grad_keys"]
    assert no_grad and all("paligemma" in k for k in no_grad)
    for k in no_grad:
        assert params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, f"{k} must not receive a gradient"
    dead = m.paligemma_with_expert.gemma_expert.lm_head.weight
    assert dead.grad is None
    with_grad = {k for k, p in params.items() if p.grad is not None and float(p.grad.abs().max()) > 0}
    assert {"state_proj.weight", "action_time_mlp_in.bias", "paligemma_with_expert.gemma_expert.model.norm.weight"} <= with_grad
    m.zero_grad(set_to_none=True)


def test_pi0_graph_replay_equals_second_replay_equals_eager(pair):
    m = pair["model"]
    m.eval()
    m._engine = None
    out = _chunk(pair)
    eng = m._engine
    assert eng is not None and eng.n_state == 1 and eng.Ss == 11 and eng._graph is not None
    out2 = _chunk(pair)  # replay_then_verify
    assert m._engine is eng and torch.equal(out, out2)
    assert not eng.stale() and not m.inference_is_stale()
    os.environ["KAI0_INFER_GRAPH"] = "0"
    try:
        m._engine = None
        out3 = _chunk(pair)
        assert m._engine._graph is None
    finally:
        os.environ.pop("KAI0_INFER_GRAPH")
        m._engine = None
    assert torch.equal(out, out3)


def test_pi0_engine_follows_weight_edits_and_keeps_an_lru(pair):
    """the fingerprint covers the pi0 heads: an optimizer-style in-place edit of state_proj rebuilds the engine; engines are cached per
    request shape."""
    from tiny import obs_to

    m, dev = pair["model"], pair["dev"]
    m.eval()
    m._engine = None
    base = _chunk(pair)
    eng = m._engine
    srcs = {id(p) for p in eng._fp_srcs}
    for p in (m.state_proj.weight, m.action_time_mlp_in.weight, m.action_time_mlp_out.bias,
              m.paligemma_with_expert.gemma_expert.model.norm.weight):  # fmt: skip
        assert id(p) in srcs
    old = m.state_proj.weight.detach().clone()
    with torch.no_grad():
        m.state_proj.weight.mul_(1.5)  # bumps the autograd version
    out = _chunk(pair)
    assert m._engine is not eng and not torch.equal(out, base)
    with torch.no_grad():
        m.state_proj.weight.copy_(old)
    assert torch.equal(_chunk(pair), base)
    # behind autograd's back: seen by the content stamp at the end of the chunk
    eng = m._engine
    m.state_proj.weight.data.mul_(1.5)
    _chunk(pair)
    torch.cuda.synchronize()
    assert eng.stale()
    m.state_proj.weight.data.copy_(old)
    m._engine = None
    assert torch.equal(_chunk(pair), base)
    # a second request shape gets an engine of its own, the first one is kept
    first = m._engine
    obs1 = copy.copy(pair["obs"])
    obs1.tokenized_prompt, obs1.tokenized_prompt_mask = obs1.tokenized_prompt[:, :16], obs1.tokenized_prompt_mask[:, :16]
    m.sample_actions(dev, obs_to(obs1, dev), noise=pair["noise"].to(dev), num_steps=10)
    assert m._engine is not first and len(m.__dict__["_engine_lru"]) == 2
    assert torch.equal(_chunk(pair), base) and m._engine is first
    m._engine = None


def test_pi0_padding_does_not_leak_and_state_matters(pair):
    from tiny import obs_to

    m, dev, obs = pair["model"], pair["dev"], pair["obs"]
    m.eval()
    base = _chunk(pair)
    tok = obs.tokenized_prompt.clone()
    tok[~obs.tokenized_prompt_mask] = 3  # rewrite only padded positions
    obs2 = copy.copy(obs)
    obs2.tokenized_prompt = tok
    assert torch.equal(base, _chunk(pair, obs_to(obs2, dev)))
    obs3 = copy.copy(obs)
    obs3.state = obs.state + 0.25
    out = _chunk(pair, obs_to(obs3, dev))  # same engine: the state is a static graph input
    assert not torch.equal(base, out) and rel(out, base) > 1e-4
    assert torch.equal(base, _chunk(pair))
    m._engine = None


def test_pi05_engine_is_untouched_by_the_state_argument():
    """pi0.5 ignores `state` as a model input (it is in the prompt): same chunk whatever is passed"""
    from tiny import build_pair, obs_to

    from oracle.pi0_oracle import synthetic_batch

    dev = torch.device("cuda:0")
    model, _, _, ocfg = build_pair(dev, seed=0, std=0.08)
    obs, _, noise, _ = synthetic_batch(ocfg, 2, seed=0)
    a = model.sample_actions(dev, obs_to(obs, dev), noise=noise.to(dev), num_steps=10)
    assert model._engine.n_state == 0 and model._engine.S == model._engine.P + 10
    obs.state = obs.state + 1.0
    assert torch.equal(a, model.sample_actions(dev, obs_to(obs, dev), noise=noise.to(dev), num_steps=10))


@pytest.mark.parametrize("n_state", [0, 1])
@pytest.mark.parametrize("Hs", [1, 10, 50])
@pytest.mark.parametrize("T", [8, 48])
@pytest.mark.parametrize("B,ncam", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_prefix_state_codes_equal_build_mask_codes_bit_for_bit(B, ncam, T, Hs, n_state):
    """kai0_prefix_state_codes (one launch) against build_mask_codes on the masks embed_prefix / embed_suffix make for
    [cams | T prompt | n_state state tokens | Hs actions] with att = [0 ... 0 | 1 x n_state | 1 0 0 ...]: equal bits, with a masked-out
    camera and a fully padded prompt; at n_state = 0 also equal to kai0_prefix_codes."""
    import ctypes as C

    from kai0_amd import _lib, ops
    from kai0_amd.model import build_mask_codes

    dev, n_img = torch.device("cuda:0"), 16
    g = torch.Generator().manual_seed(B * 131 + ncam * 17 + T)
    img_masks = [torch.ones(B, dtype=torch.bool) for _ in range(ncam)]
    img_masks[-1][0] = False  # a masked-out camera
    lang = torch.rand(B, T, generator=g) > 0.35
    lang[0] = torch.arange(T) < max(1, T // 2)
    lang[-1] = False  # a fully padded prompt (at B = 1: with the masked-out camera)
    img_masks, lang = [m.to(dev) for m in img_masks], lang.to(dev)
    P, Ss = ncam * n_img + T, n_state + Hs
    pad = torch.cat([m[:, None].expand(B, n_img) for m in img_masks] + [lang, torch.ones(B, Ss, dtype=torch.bool, device=dev)], dim=1)
    att = torch.zeros(B, P + Ss, dtype=torch.bool, device=dev)
    att[:, P : P + n_state + 1] = True
    want = build_mask_codes(pad, att)
    q, k, p = (torch.full((B, P + Ss), -7, dtype=torch.int32, device=dev) for _ in range(3))
    ptrs = (C.c_void_p * ncam)(*[m.data_ptr() for m in img_masks])
    _lib.call("kai0_prefix_state_codes", C.addressof(ptrs), ncam, lang.data_ptr(), B, n_img, T, n_state, Hs, q.data_ptr(), k.data_ptr(),
              p.data_ptr(), ops._stream())  # fmt: skip
    for a, b, name in zip((q, k, p), want, ("qcode", "kcode", "pos")):
        assert torch.equal(a, b), name
    for a, b in zip(ops.prefix_codes(img_masks, lang, n_img, Hs, n_state=n_state), want):
        assert a.dtype == torch.int32 and torch.equal(a, b)
    if n_state == 0:
        for a, b in zip((q, k, p), ops.prefix_codes(img_masks, lang, n_img, Hs)):
            assert torch.equal(a, b)


def test_train_loop_debug_pi0_checkpoints_and_resumes_exactly(tmp_path):
    """`train_loop(get_config("debug"))` (the registry's pi0 entry): 4 steps write a checkpoint; stopped after 2 and resumed, steps 2
    and 3 log the same loss, learning rate and gradient norm (test_train_loop_debug_pi05_resume_is_exact's criteria)."""
    import dataclasses as dc

    from kai0_amd import training_config as tc
    from kai0_amd.train import train_loop

    cfg = tc.get_config("debug")
    assert cfg.model.pi05 is False and cfg.model.model_type == "pi0"
    base = dc.replace(cfg, checkpoint_base_dir=str(tmp_path / "ckpt"), assets_base_dir=str(tmp_path / "assets"),
                      num_workers=0, num_train_steps=4, log_interval=1, save_interval=100,
                      lr_schedule=tc.CosineDecaySchedule(warmup_steps=2, peak_lr=1e-3, decay_steps=10, decay_lr=1e-4))  # fmt: skip
    full = train_loop(dc.replace(base, exp_name="full", overwrite=True))
    assert [r["step"] for r in full] == list(range(4)) and all(r["loss"] == r["loss"] for r in full)
    assert sorted(os.listdir(tmp_path / "ckpt" / "debug" / "full" / "4")) == ["metadata.pt", "model.safetensors", "optimizer.pt"]
    keys = set(load_file(str(tmp_path / "ckpt" / "debug" / "full" / "4" / "model.safetensors")))
    assert "state_proj.weight" in keys and "action_time_mlp_in.weight" in keys and "time_mlp_in.weight" not in keys
    part = train_loop(dc.replace(base, exp_name="cut", num_train_steps=2, overwrite=True))
    assert [r["loss"] for r in part] == [r["loss"] for r in full[:2]]
    rest = train_loop(dc.replace(base, exp_name="cut", overwrite=False, resume=True))
    assert [r["step"] for r in rest] == [2, 3]
    for a, b in zip(rest, full[2:]):
        assert a["loss"] == b["loss"] and a["grad_norm"] == b["grad_norm"] and a["learning_rate"] == b["learning_rate"], (a, b)
    print("debug (pi0) loss curve", [round(r["loss"], 5) for r in full])


def test_pi0_policy_from_a_pi0_config_serves_a_request(tmp_path):
    """`create_trained_policy(train_config, checkpoint_dir)` with a pi0 model config (tests/test_model_gpu.py's serve-path test, pi0):
    the pi0 transform stack (z-score normalisation, the prompt tokenised WITHOUT the state, 48 slots), the state as a model input of the
    captured graph; the robot actions against the CPU restatement fed with the same transformed observation and noise."""
    import pi0_restatement as R
    from test_training_config_cpu import _agilex_cfg, _checkpoint
    from tiny import tiny_cfgs

    from kai0_amd import policy as _policy
    from kai0_amd.preprocessing import Observation, preprocess_observation
    from oracle.pi0_oracle import SimpleObs

    cfg = _agilex_cfg(use_delta_joint_actions=False)
    cfg = dataclasses.replace(cfg, model=dataclasses.replace(cfg.model, pi05=False, max_token_len=48, discrete_state_input=None))
    assert cfg.model.model_type == "pi0" and cfg.model.discrete_state_input is False
    model, ck, _ = _checkpoint(tmp_path, cfg, seed=9)
    pol = _policy.create_trained_policy(cfg, ck, sample_kwargs={"num_steps": 10}, pytorch_device="cuda:0")
    names = [type(t).__name__ for t in pol._input_transform.transforms]
    tok = pol._input_transform.transforms[names.index("TokenizePrompt")]
    norm = pol._input_transform.transforms[names.index("Normalize")]
    assert not tok.discrete_state_input and not norm.use_quantiles
    rng = np.random.default_rng(1)
    cams = {k: rng.integers(0, 256, size=(3, 48, 64), dtype=np.uint8) for k in ("top_head", "hand_left", "hand_right")}
    state = rng.uniform(-1.0, 1.0, size=14)
    noise = rng.normal(size=(10, 32)).astype(np.float32)
    raw = {"images": cams, "state": state, "prompt": "fold the cloth"}
    res = pol.infer(dict(raw), noise=noise)
    assert res["actions"].shape == (10, 14) and np.isfinite(res["actions"]).all()
    assert np.array_equal(res["actions"], pol.infer(dict(raw), noise=noise)["actions"])  # replayed
    other = pol.infer({**raw, "state": state + 0.2}, noise=noise)["actions"]
    assert not np.array_equal(res["actions"], other)  # the state reaches the model
    # the restatement on the same transformed inputs
    _, ocfg05 = tiny_cfgs(max_token_len=48)
    ref_model = R.RestatedPI0(R.pi0_cfg(ocfg05))
    ref_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=True)
    inp = pol._input_transform(dict(raw))
    assert inp["tokenized_prompt"].shape == (48,)
    batched = {k: ({kk: torch.from_numpy(np.asarray(vv))[None] for kk, vv in v.items()} if isinstance(v, dict)
                   else torch.from_numpy(np.asarray(v))[None]) for k, v in inp.items()}  # fmt: skip
    obs = preprocess_observation(Observation.from_dict(batched), train=False, image_resolution=(56, 56))
    sobs = SimpleObs(images=dict(obs.images), image_masks=dict(obs.image_masks), state=obs.state, tokenized_prompt=obs.tokenized_prompt,
                     tokenized_prompt_mask=obs.tokenized_prompt_mask, token_ar_mask=None, token_loss_mask=None)  # fmt: skip
    with torch.no_grad():
        ref = ref_model.eval().sample_actions(sobs, torch.from_numpy(noise)[None], num_steps=10)
    want = pol._output_transform({"state": inp["state"], "actions": ref[0].numpy()})["actions"]
    err = np.abs(res["actions"] - want).max() / (np.abs(want).max() + 1e-9)
    print(f"pi0 Policy.infer vs restatement: max rel err {err:.3e}")
    assert err < 2e-2  # tests/test_model_gpu.py::test_policy_infer_over_the_hip_model's bound
