"""Real-time chunking on the HIP engine (infer.InferenceEngine.sample_actions_guided) against the CPU restatement
(tests/rtc_restatement.py: the oracle's blocks + torch.autograd.grad), on the tiny pair (std 0.05, B = 2, Hs = 10) and at full width,
depth 2 (B = 1, Hs = 50, P = 968: the real widths, 1018 keys, the logits / softmax / P V attention branch).

Bounds.  The VJP is held to the project's rule for gradients: rel-L2(HIP, f32) <= 1.5 x rel-L2(bf16 restatement, f32) + 2e-3, both
measured here on the same x_t and cotangent.  The guided chunk carries the unguided chunk's bounds against the f32 restatement
(rel-L2 <= 3e-3, max|d| <= 2e-2: the bf16 floor is the same, 7.3e-4 for the bf16 restatement on the tiny case), and must differ from
the unguided chunk by >= 0.1 rel-L2 and be strictly closer to the previous chunk where it is steered — so that none of this passes
with the guidance doing nothing.  Measured values: DESIGN.md section 5, profiles/HISTORY.md."""

import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

F32 = torch.float32
CASES = {"tiny": dict(inference_delay=2, execute_horizon=6), "fullwidth": dict(inference_delay=3, execute_horizon=8)}


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def _references(oracle, o32, obs, noise, prev, case):
    """Everything the CPU computes, once per model: unguided and guided f32 chunks (default cap and 2.5) with the f32 trace, and the
    bf16 restatement's VJP at the f32 trace's first and last steps."""
    import rtc_restatement as R

    kw = dict(prev_action_chunk=prev, prefix_attention_schedule="exp", **case)
    trace = []
    out = dict(plain=o32.sample_actions(obs, noise, num_steps=10), guided=R.sample_actions(o32, obs, noise, 10, trace=trace, **kw),
               guided25=R.sample_actions(o32, obs, noise, 10, max_guidance_weight=2.5, **kw), steps={})  # fmt: skip
    ppad, cache = R.prefix_cache(oracle, obs)
    for step in (0, 9):
        x_t, t, _, e, corr32 = trace[step]
        _, _, _, corr_bf = R.x1_and_vjp(oracle, ppad, cache, x_t, torch.tensor(t, dtype=F32), lambda x1, e=e: e)
        out["steps"][step] = dict(x_t=x_t, t=t, e=e, corr32=corr32, corr_bf=corr_bf)
    return out


@pytest.fixture(scope="module")
def tiny():
    from tiny import build_pair, obs_to

    from oracle.pi0_oracle import synthetic_batch

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    model, oracle, _, ocfg = build_pair(dev(), std=0.05)
    o32 = copy.deepcopy(oracle)
    o32.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    obs, actions, noise, _ = synthetic_batch(ocfg, 2, seed=0)
    prev = torch.zeros_like(actions)
    prev[..., :14] = actions[..., :14]
    model.eval()
    return dict(name="tiny", model=model, obs=obs, gobs=obs_to(obs, dev()), noise=noise, prev=prev, case=CASES["tiny"],
                ref=_references(oracle.eval(), o32.eval(), obs, noise, prev, CASES["tiny"]))  # fmt: skip


@pytest.fixture(scope="module")
def fullwidth():
    from fullwidth import build_hip, build_oracle
    from tiny import obs_to

    from oracle.pi0_oracle import synthetic_batch

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    oracle, ocfg = build_oracle(2, 2)
    model = build_hip(oracle, 2, 2, dev())
    o32 = copy.deepcopy(oracle)
    o32.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    obs, actions, noise, _ = synthetic_batch(ocfg, 1, seed=3)
    prev = torch.zeros_like(actions)
    prev[..., :14] = actions[..., :14]
    model.eval()
    return dict(name="fullwidth", model=model, obs=obs, gobs=obs_to(obs, dev()), noise=noise, prev=prev, case=CASES["fullwidth"],
                ref=_references(oracle.eval(), o32.eval(), obs, noise, prev, CASES["fullwidth"]))  # fmt: skip


@pytest.fixture(params=["tiny", "fullwidth"])
def pair(request):
    return request.getfixturevalue(request.param)


def _engine(model, gobs, noise):
    """the engine of this request shape (built by an unguided call) and the preprocessed request"""
    model.sample_actions(dev(), gobs, noise=noise.to(dev()), num_steps=10)
    images, img_masks, lang_tokens, lang_masks, _ = model._preprocess_observation(gobs, train=False)
    return model._engine, (images, img_masks, lang_tokens, lang_masks)


@pytest.mark.parametrize("step", [0, 9])
def test_denoiser_vjp_against_f32_restatement(pair, step):
    m, s = pair["model"], pair["ref"]["steps"][step]
    eng, req = _engine(m, pair["gobs"], pair["noise"])
    _, jte = eng.denoiser_vjp(*req, s["x_t"].to(dev()), s["e"].to(dev()), 10, step)
    corr = s["e"] - torch.tensor(s["t"], dtype=F32) * jte.cpu()
    r_hip, r_bf = rel(corr, s["corr32"]), rel(s["corr_bf"], s["corr32"])
    print(f"{pair['name']} VJP step {step} (t = {s['t']:.1f}): rel-L2 HIP vs f32 {r_hip:.3e}, bf16 restatement vs f32 {r_bf:.3e}")
    assert torch.isfinite(corr).all()
    assert r_hip <= 1.5 * r_bf + 2e-3


@pytest.mark.parametrize("cap", [0.5, 2.5])
def test_guided_chunk_against_f32_restatement(pair, cap):
    m, d, ref, prev = pair["model"], dev(), pair["ref"], pair["prev"]
    noise = pair["noise"].to(d)
    plain = m.sample_actions(d, pair["gobs"], noise=noise, num_steps=10)
    out = m.sample_actions(d, pair["gobs"], noise=noise, num_steps=10, prev_action_chunk=prev, prefix_attention_schedule="exp",
                           max_guidance_weight=cap, **pair["case"])  # fmt: skip
    want = ref["guided"] if cap == 0.5 else ref["guided25"]
    r, mx, moved = rel(out, want), float((out.cpu() - want).abs().max()), rel(out, plain)
    print(f"{pair['name']} guided chunk, cap {cap}: rel-L2 {r:.3e}, max|d| {mx:.3e} vs f32 restatement; vs HIP unguided {moved:.3e} "
          f"(f32 restatement: guided vs unguided {rel(want, ref['plain']):.3e})")
    assert out.shape == noise.shape and out.dtype == F32 and torch.isfinite(out).all()
    assert r <= 3e-3 and mx <= 2e-2
    assert moved >= 0.1
    eh = pair["case"]["execute_horizon"]
    sl = (slice(None), slice(0, eh), slice(0, 14))
    assert (out.cpu()[sl] - prev[sl]).norm() < (plain.cpu()[sl] - prev[sl]).norm()


# ------------------------------------------------------------------------------------------------ identities (generic engine)
@pytest.fixture()
def generic(tiny):
    from kai0_amd.infer import InferenceEngine

    m = tiny["model"]
    old = InferenceEngine.force_generic
    InferenceEngine.force_generic = True
    m.invalidate_inference_engine()
    try:
        yield tiny
    finally:
        InferenceEngine.force_generic = old
        m.invalidate_inference_engine()


def test_zero_weights_and_disabled_guidance_are_the_unguided_chunk(generic):
    m, d = generic["model"], dev()
    gobs, noise, prev = generic["gobs"], generic["noise"].to(d), generic["prev"]
    plain = m.sample_actions(d, gobs, noise=noise, num_steps=10)
    eng, graph = m._engine, m._engine._graph
    assert not eng.fast and graph is not None
    zero = m.sample_actions(d, gobs, noise=noise, num_steps=10, prev_action_chunk=prev, inference_delay=0, execute_horizon=6,
                            prefix_attention_schedule="zeros")  # fmt: skip
    assert torch.equal(zero, plain)
    off = m.sample_actions(d, gobs, noise=noise, num_steps=10, prev_action_chunk=prev, enable_rtc=False, **generic["case"])
    none = m.sample_actions(d, gobs, noise=noise, num_steps=10, prev_action_chunk=None, **generic["case"])
    assert torch.equal(off, plain) and torch.equal(none, plain)
    assert m._engine is eng and eng._graph is graph  # the unguided graph is the one captured before the guided call


def test_guided_graph_equals_guided_eager_and_touches_no_weight(generic):
    m, d = generic["model"], dev()
    gobs, noise = generic["gobs"], generic["noise"].to(d)
    kw = dict(prev_action_chunk=generic["prev"], prefix_attention_schedule="exp", **generic["case"])
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    replayed = m.sample_actions(d, gobs, noise=noise, num_steps=10, **kw)
    eng = m._engine
    assert eng._g_graph is not None, "the guided chunk was not captured"
    assert torch.equal(m.sample_actions(d, gobs, noise=noise, num_steps=10, **kw), replayed)  # a second replay
    eng.use_graph = False
    try:
        eager = m.sample_actions(d, gobs, noise=noise, num_steps=10, **kw)
    finally:
        eng.use_graph = True
    assert torch.equal(eager, replayed)
    torch.cuda.synchronize()
    assert not m.inference_is_stale()
    for n, p in m.named_parameters():
        assert p.grad is None, n
        assert torch.equal(p.detach(), before[n]), n


def test_policy_serves_the_guided_chunk(tiny):
    from kai0_amd.policy import Policy

    m, d, obs = tiny["model"], dev(), tiny["obs"]
    pol = Policy(m, pytorch_device="cuda:0", device_resize=False)
    req = {"image": {k: v[0].numpy() for k, v in obs.images.items()}, "image_mask": {k: v[0].numpy() for k, v in obs.image_masks.items()},
           "state": obs.state[0].numpy(), "tokenized_prompt": obs.tokenized_prompt[0].numpy(),
           "tokenized_prompt_mask": obs.tokenized_prompt_mask[0].numpy()}  # fmt: skip
    noise = tiny["noise"][0].numpy()
    prev14 = tiny["prev"][0, :, :14]
    guided = pol.infer({**req, "prev_action_chunk": prev14.tolist(), "inference_delay": 2, "execute_horizon": 6}, noise=noise)["actions"]
    plain = pol.infer(req, noise=noise)["actions"]
    from kai0_amd.preprocessing import slice_observation

    g1 = slice_observation(tiny["gobs"], 0, 1)
    n1 = tiny["noise"][0:1].to(d)
    want_g = m.sample_actions(d, g1, noise=n1, num_steps=10, prev_action_chunk=prev14, inference_delay=2, execute_horizon=6)
    want_p = m.sample_actions(d, g1, noise=n1, num_steps=10)
    assert np.array_equal(guided, want_g[0].cpu().numpy()) and np.array_equal(plain, want_p[0].cpu().numpy())
    assert not np.array_equal(guided, plain)
