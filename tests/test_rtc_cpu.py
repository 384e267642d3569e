"""Real-time chunking, host side (kai0_amd/rtc.py, the request surface of model.sample_actions and Policy.infer) and the CPU
restatement the GPU tests are held against (tests/rtc_restatement.py).  The reference is JAX and is not executed here: the pins
below are hand-computed from pi0_rtc.py:47-61 and :340-346."""

import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from kai0_amd import rtc  # noqa: E402


# ------------------------------------------------------------------------------------------------ prefix weights, guidance weight
@pytest.mark.parametrize("schedule,expected", [
    ("ones", [1, 1, 1, 1, 1, 1, 0, 0, 0, 0]),
    ("zeros", [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]),
    ("linear", [1, 1, 0.8, 0.6, 0.4, 0.2, 0, 0, 0, 0]),
    ("exp", [1, 1, 0.570589, 0.287072, 0.114492, 0.025770, 0, 0, 0, 0]),
])  # fmt: skip
def test_prefix_weights_pins(schedule, expected):
    w = rtc.get_prefix_weights(2, 6, 10, schedule)
    assert w.dtype == np.float32 and w.shape == (10,)
    np.testing.assert_allclose(w, np.asarray(expected, dtype=np.float32), rtol=0, atol=2e-6)


def test_prefix_weights_edges():
    assert not rtc.get_prefix_weights(0, 6, 10, "zeros").any()
    np.testing.assert_array_equal(rtc.get_prefix_weights(7, 6, 10, "exp"), np.asarray([1] * 6 + [0] * 4, dtype=np.float32))
    with pytest.raises(ValueError):
        rtc.get_prefix_weights(2, 6, 10, "cosine")


def test_guidance_weights_at_ten_steps():
    from kai0_amd.infer import euler_times

    times = euler_times(10)
    assert len(times) == 10
    free = rtc.guidance_weights(times, 1e9)
    np.testing.assert_allclose(free, [999.0, 9.1111, 4.25, 2.7619, 2.1667, 2.0, 2.1667, 2.7619, 4.25, 9.1111], rtol=2e-4)
    assert rtc.guidance_weights(times, 0.5) == [0.5] * 10
    mixed = rtc.guidance_weights(times, 2.5)  # the cap at which the formula matters: steps 4 .. 6 are below it
    assert mixed[:4] == [2.5] * 4 and mixed[7:] == [2.5] * 3 and all(2.0 - 1e-3 <= g < 2.5 for g in mixed[4:7])


# ------------------------------------------------------------------------------------------------ argument handling
def test_resolve_arguments():
    H, A = 10, 32
    prev = np.arange(H * 20, dtype=np.float32).reshape(H, 20)
    prev[3, 4], prev[0, 0], prev[9, 19] = np.nan, np.inf, -np.inf
    gd = rtc.resolve(prev.tolist(), batch=2, action_horizon=H, action_dim=A, inference_delay=2, execute_horizon=6)
    assert gd.prev.shape == (2, H, A) and gd.prev.dtype == np.float32 and gd.provided == 14
    assert gd.prev[1, 3, 4] == 0 and gd.prev[0, 0, 0] == 0 and gd.prev[0, 9, 19] == 0 and not gd.prev[..., 20:].any()
    assert gd.prev[1, 5, 7] == prev[5, 7]
    np.testing.assert_array_equal(gd.weights, rtc.get_prefix_weights(2, 6, H, "exp"))
    wide = rtc.resolve(np.ones((1, H, 40), dtype=np.float32), batch=1, action_horizon=H, action_dim=A)
    assert wide.prev.shape == (1, H, A) and wide.provided == 14
    np.testing.assert_array_equal(wide.weights, rtc.get_prefix_weights(0, H, H, "exp"))  # no delay, the whole horizon
    assert rtc.resolve(np.ones((H, 7)), batch=1, action_horizon=H, action_dim=A).provided == 7
    np.testing.assert_array_equal(rtc.resolve(np.ones((H, 7)), batch=1, action_horizon=H, action_dim=A, inference_delay=99,
                                              execute_horizon=99).weights, np.ones(H, dtype=np.float32))  # both clipped to H
    with pytest.raises(ValueError):
        rtc.resolve(np.ones((H + 1, A)), batch=1, action_horizon=H, action_dim=A)
    with pytest.raises(ValueError):
        rtc.resolve(np.ones((H, A)), batch=1, action_horizon=H, action_dim=A, prefix_attention_schedule="cosine")


def _cpu_model(pi05: bool):
    import dataclasses

    from tiny import tiny_cfgs

    from kai0_amd.model import PI0Pytorch
    from oracle.pi0_oracle import synthetic_batch

    pcfg, ocfg = tiny_cfgs()
    obs, actions, noise, _ = synthetic_batch(ocfg, 1, seed=0)
    return PI0Pytorch(pcfg if pi05 else dataclasses.replace(pcfg, pi05=False)), obs, actions, noise


def test_model_refusals_and_bad_horizon():
    """Raised before any device work: checked on a CPU-resident model."""
    m, obs, actions, noise = _cpu_model(True)
    with pytest.raises(NotImplementedError):
        m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0], mask_prefix_delay=True)
    with pytest.raises(ValueError):
        m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0, :-1])
    with pytest.raises(ValueError):
        m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0], prefix_attention_schedule="cosine")
    m0, obs, actions, noise = _cpu_model(False)
    with pytest.raises(NotImplementedError):
        m0.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0])


# ------------------------------------------------------------------------------------------------ Policy
class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = []

    def sample_actions(self, device, observation, **kw):
        self.calls.append(kw)
        return torch.zeros((1, 10, 32))


class _Spy:
    def __init__(self):
        self.seen = []

    def __call__(self, data):
        self.seen.append(set(data))
        return data


def _request(**extra):
    return {"image": {"base_0_rgb": np.zeros((8, 8, 3), dtype=np.float32)}, "image_mask": {"base_0_rgb": np.True_},
            "state": np.zeros(32, dtype=np.float32), "tokenized_prompt": np.zeros(4, dtype=np.int32),
            "tokenized_prompt_mask": np.ones(4, dtype=bool), **extra}  # fmt: skip


def test_policy_passes_exactly_the_three_keys():
    from kai0_amd.policy import Policy

    stub, spy = _StubModel(), _Spy()
    pol = Policy(stub, transforms=[spy], pytorch_device="cpu", device_resize=False)
    chunk = np.arange(10 * 14, dtype=np.float32).reshape(10, 14)
    pol.infer(_request(prev_action_chunk=chunk.tolist(), inference_delay=3, execute_horizon=[8]))
    pol.infer(_request())
    guided, plain = stub.calls
    assert set(guided) == {"prev_action_chunk", "inference_delay", "execute_horizon"}
    np.testing.assert_array_equal(guided["prev_action_chunk"], chunk)  # raw, as the reference hands it on
    assert guided["inference_delay"] == 3 and guided["execute_horizon"] == 8
    assert plain == {}
    assert all(not (s & {"prev_action_chunk", "inference_delay", "execute_horizon"}) for s in spy.seen) and len(spy.seen) == 2


@pytest.mark.parametrize("quant", [False, True])
def test_policy_rtc_normalize_prev(quant):
    from kai0_amd import normalize, transforms
    from kai0_amd.policy import Policy

    rng = np.random.default_rng(0)
    stats = normalize.NormStats(mean=rng.normal(size=14), std=rng.uniform(0.5, 2, size=14), q01=-rng.uniform(1, 2, size=14),
                                q99=rng.uniform(1, 2, size=14))  # fmt: skip
    un = transforms.Unnormalize({"actions": stats}, use_quantiles=quant)
    stub = _StubModel()
    pol = Policy(stub, output_transforms=[un], pytorch_device="cpu", device_resize=False, rtc_normalize_prev=True)
    chunk = rng.normal(size=(10, 14)).astype(np.float32)
    pol.infer(_request(prev_action_chunk=chunk.tolist()))
    got = stub.calls[0]["prev_action_chunk"]
    np.testing.assert_allclose(got, normalize.normalize(chunk, stats, use_quantiles=quant), rtol=1e-6, atol=1e-6)
    # ... and it is the inverse of what the output stack does to the model's chunk
    np.testing.assert_allclose(normalize.unnormalize(got.astype(np.float64), stats, use_quantiles=quant), chunk, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        Policy(stub, output_transforms=[un, transforms.AbsoluteActions(None)], pytorch_device="cpu", device_resize=False,
               rtc_normalize_prev=True)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def tiny32():
    from tiny import tiny_cfgs

    from oracle.pi0_oracle import OraclePI0, synthetic_batch, synthetic_weights_

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    _, ocfg = tiny_cfgs()
    oracle = OraclePI0(ocfg)
    synthetic_weights_(oracle, seed=0)
    with torch.no_grad():
        for _, p in oracle.named_parameters():
            if p.dim() >= 2:
                p.mul_(0.05 / 0.02)
    o32 = copy.deepcopy(oracle)
    o32.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    obs, actions, noise, _ = synthetic_batch(ocfg, 2, seed=0)
    return dict(oracle=oracle.eval(), o32=o32.eval(), obs=obs, actions=actions, noise=noise)


def _prev(actions):
    prev = torch.zeros_like(actions)
    prev[..., :14] = actions[..., :14]
    return prev


def test_restatement_without_previous_chunk_is_the_oracle(tiny32):
    import rtc_restatement as R

    for o in (tiny32["oracle"], tiny32["o32"]):
        ref = o.sample_actions(tiny32["obs"], tiny32["noise"], num_steps=10)
        assert torch.equal(R.sample_actions(o, tiny32["obs"], tiny32["noise"], 10), ref)
        assert torch.equal(R.sample_actions(o, tiny32["obs"], tiny32["noise"], 10, prev_action_chunk=_prev(tiny32["actions"]),
                                            enable_rtc=False), ref)  # fmt: skip


def test_restatement_vjp_matches_float64_finite_difference(tiny32):
    """<(dx1/dx)^T e, d> of the f32 restatement = <e, (x1(x + h d) - x1(x - h d)) / 2h> of the float64 oracle, three directions.
    f32 autograd against an f64 central difference at h = 1e-4: truncation ~h^2, model precision ~1e-6 -> 1e-3 relative is ample."""
    import rtc_restatement as R

    o32 = tiny32["o32"]
    o64 = copy.deepcopy(o32).double()
    obs, x = tiny32["obs"], tiny32["noise"]
    g = torch.Generator().manual_seed(1)
    e = torch.randn(x.shape, generator=g)
    t = torch.tensor(0.7, dtype=torch.float32)
    ppad, cache = R.prefix_cache(o32, obs)
    _, _, _, corr = R.x1_and_vjp(o32, ppad, cache, x, t, lambda x1: e)
    obs64 = copy.copy(obs)
    obs64.images = {k: v.double() for k, v in obs.images.items()}
    ppad64, cache64 = R.prefix_cache(o64, obs64)
    h, t64 = 1e-4, t.double()
    for _ in range(3):
        d = torch.randn(x.shape, generator=g)
        with torch.no_grad():
            xp, xm = x.double() + h * d.double(), x.double() - h * d.double()
            x1p = xp - t64 * R.velocity(o64, ppad64, cache64, xp, t64)
            x1m = xm - t64 * R.velocity(o64, ppad64, cache64, xm, t64)
        fd = float(((x1p - x1m) / (2 * h) * e.double()).sum())
        got = float((corr.double() * d.double()).sum())
        assert abs(got - fd) <= 1e-3 * abs(fd) + 1e-6, (got, fd)


def test_restatement_guided_chunk_is_finite_steered_and_bf16_close(tiny32):
    """d = 2, exec_h = 6, "exp": the guided f32 chunk differs from the unguided one and is closer to prev where it is steered; the
    cap 2.5 (the formula matters) keeps it finite; the bf16 restatement stays at the unguided chunk's bf16 floor."""
    import rtc_restatement as R

    o32, obs, noise = tiny32["o32"], tiny32["obs"], tiny32["noise"]
    prev = _prev(tiny32["actions"])
    kw = dict(prev_action_chunk=prev, inference_delay=2, execute_horizon=6, prefix_attention_schedule="exp")
    plain = o32.sample_actions(obs, noise, num_steps=10)
    g32 = R.sample_actions(o32, obs, noise, 10, **kw)
    gb = R.sample_actions(tiny32["oracle"], obs, noise, 10, **kw)
    g25 = R.sample_actions(o32, obs, noise, 10, max_guidance_weight=2.5, **kw)
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    assert torch.isfinite(g32).all() and torch.isfinite(g25).all() and torch.isfinite(gb).all()
    print(f"guided vs unguided {rel(g32, plain):.3e}; bf16 vs f32 guided {rel(gb, g32):.3e}; cap 2.5 vs unguided {rel(g25, plain):.3e}")
    assert rel(g32, plain) >= 0.1
    sl = (slice(None), slice(0, 6), slice(0, 14))
    assert (g32[sl] - prev[sl]).norm() < (plain[sl] - prev[sl]).norm()
    assert rel(gb, g32) <= 3e-3
    zero = R.sample_actions(o32, obs, noise, 10, prev_action_chunk=prev, inference_delay=0, execute_horizon=6,
                            prefix_attention_schedule="zeros")  # fmt: skip
    assert torch.equal(zero, plain)  # all-zero weights: the guidance does nothing
