"""Real-time chunking for pi0 (`pi05=False`) and `mask_prefix_delay`, without a GPU: the CPU restatements the GPU tests are held against
(tests/rtc_restatement.py over tests/pi0_restatement.RestatedPI0, tests/rtc_delay_restatement.py), the host side (kai0_amd/rtc.py, the
request surface of model.sample_actions) and the new export's declaration.  The reference is JAX and is not executed here: the delay
branch is pinned on a one-step case worked out by hand from pi0_rtc.py:322-349."""

import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from kai0_amd import rtc  # noqa: E402


def rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def tiny10():
    import rtc_pi0_cases as cases

    return cases.tiny_pi0(10)


# ------------------------------------------------------------------------------------------------ the pi0 restatement
def test_pi0_restatement_without_previous_chunk_is_the_restated_model(tiny10):
    import rtc_delay_restatement as D
    import rtc_restatement as R

    obs, noise = tiny10["obs"], tiny10["noise"]
    for o in (tiny10["ref"], tiny10["ref32"]):
        want = o.sample_actions(obs, noise, num_steps=10)  # (sets o._state)
        assert torch.equal(R.sample_actions(o, obs, noise, 10), want)
        assert torch.equal(R.sample_actions(o, obs, noise, 10, prev_action_chunk=tiny10["prev"], enable_rtc=False), want)
        for flag in (False, True):  # the flag does nothing without a previous chunk, or with enable_rtc=False (:351)
            assert torch.equal(D.sample_actions(o, obs, noise, 10, mask_prefix_delay=flag), want)
            assert torch.equal(D.sample_actions(o, obs, noise, 10, prev_action_chunk=tiny10["prev"], enable_rtc=False,
                                                mask_prefix_delay=flag), want)  # fmt: skip


def test_pi0_restatement_vjp_matches_float64_finite_difference(tiny10):
    """<(dx1/dx)^T e, d> of the f32 pi0 restatement = <e, (x1(x + h d) - x1(x - h d)) / 2h> of the float64 RestatedPI0, three directions
    (tests/test_rtc_cpu.py's check for pi0.5, same bound): the Jacobian here also runs through action_time_mlp_in / SiLU /
    action_time_mlp_out, and must NOT run through the state token.
    h = 1e-3, not that test's 1e-4: the oracle's RMSNorm takes its variance (and, on the plain path pi0 uses, 1 + w) in float32 whatever
    the model's dtype (pi0_oracle.py GemmaRMSNorm), so the "float64" model carries f32 noise, ~1e-7 |x1| / h in the difference quotient:
    measured against float64 autograd, the quotient is off by 6e-3 / 2e-4 / 5e-5 relative at h = 1e-5 / 1e-4 / 1e-3 (truncation ~h^2
    is still below 1e-5 there).  The float64 autograd VJP itself is a second arbiter: the f32 one must agree with it to 1e-5."""
    import rtc_restatement as R

    r32, obs, x = tiny10["ref32"], tiny10["obs"], tiny10["noise"]
    r32._state = obs.state
    o64 = copy.deepcopy(r32).double()
    o64._state = obs.state.double()
    g = torch.Generator().manual_seed(1)
    e = torch.randn(x.shape, generator=g)
    t = torch.tensor(0.7, dtype=torch.float32)
    ppad, cache = R.prefix_cache(r32, obs)
    _, _, _, corr = R.x1_and_vjp(r32, ppad, cache, x, t, lambda x1: e)
    obs64 = copy.copy(obs)
    obs64.images = {k: v.double() for k, v in obs.images.items()}
    ppad64, cache64 = R.prefix_cache(o64, obs64)
    _, _, _, corr64 = R.x1_and_vjp(o64, ppad64, cache64, x.double(), t.double(), lambda x1: e.double())
    assert rel(corr.double(), corr64) <= 1e-5
    h, t64 = 1e-3, t.double()
    for _ in range(3):
        d = torch.randn(x.shape, generator=g)
        with torch.no_grad():
            xp, xm = x.double() + h * d.double(), x.double() - h * d.double()
            x1p = xp - t64 * R.velocity(o64, ppad64, cache64, xp, t64)
            x1m = xm - t64 * R.velocity(o64, ppad64, cache64, xm, t64)
        fd = float(((x1p - x1m) / (2 * h) * e.double()).sum())
        got = float((corr.double() * d.double()).sum())
        assert abs(got - fd) <= 1e-3 * abs(fd) + 1e-6, (got, fd)


@pytest.mark.parametrize("horizon", [10, 16])
def test_pi0_restatement_guided_chunk_moves_far_enough(horizon, tiny10):
    """The condition the GPU test's `>= 0.1 from the unguided chunk` rests on: the f32 restatement's own guided-vs-unguided distance is
    >= 0.15 at every (case, cap) used, it is steered towards prev, and the bf16 restatement stays at the unguided chunk's bf16 floor.
    Measured: Hs = 10: 0.193 / 0.490 (cap 0.5 / 2.5); Hs = 16 (prev = 1.5 x actions): 0.187 / 0.479; full width (B = 1, Hs = 50, checked
    when the inputs were fixed, too slow for this suite): see tests/test_rtc_pi0_gpu.py."""
    import rtc_pi0_cases as cases

    case = tiny10 if horizon == 10 else cases.tiny_pi0(16)
    name = f"tiny{horizon}"
    ref = cases.references(case, cases.RTC[name], steps=())
    eh = cases.RTC[name]["execute_horizon"]
    sl = (slice(None), slice(0, eh), slice(0, 14))
    for cap in cases.CAPS:
        g = ref["guided"][cap]
        moved = rel(g, ref["plain"])
        print(f"{name} cap {cap}: f32 restatement guided vs unguided {moved:.3e}")
        assert torch.isfinite(g).all() and moved >= 0.15
        assert (g[sl] - case["prev"][sl]).norm() < (ref["plain"][sl] - case["prev"][sl]).norm()
    import rtc_restatement as R

    gb = R.sample_actions(case["ref"], case["obs"], case["noise"], 10, prev_action_chunk=case["prev"], **cases.RTC[name])
    assert rel(gb, ref["guided"][0.5]) <= 3e-3


# ------------------------------------------------------------------------------------------------ mask_prefix_delay
def test_delay_restatement_d0_is_the_flag_off(tiny10):
    import rtc_delay_restatement as D
    import rtc_restatement as R

    r32, obs, noise, prev = tiny10["ref32"], tiny10["obs"], tiny10["noise"], tiny10["prev"]
    kw = dict(prev_action_chunk=prev, execute_horizon=6)
    off = D.sample_actions(r32, obs, noise, 10, inference_delay=2, **kw)
    assert torch.equal(off, R.sample_actions(r32, obs, noise, 10, inference_delay=2, **kw))  # flag off: rtc_restatement's loop
    for d in (0, None):
        assert torch.equal(D.sample_actions(r32, obs, noise, 10, inference_delay=d, mask_prefix_delay=True, **kw),
                           D.sample_actions(r32, obs, noise, 10, inference_delay=d, **kw))  # fmt: skip
    on = D.sample_actions(r32, obs, noise, 10, inference_delay=2, mask_prefix_delay=True, **kw)
    assert torch.isfinite(on).all() and not torch.equal(on, off)


def test_delay_restatement_one_step_by_hand(tiny10):
    """num_steps = 1: t = 1, dt = -1, g = min(999 * (0.999^2 + 1e-6) / 0.999^2, 0.5) = 0.5.  With d = 3 and 14 provided columns:
        x_den = prev on rows 0..2, columns 0..13; noise elsewhere                          (:324-327)
        v, x1 = x_den - v, e = (prev - x1) w mask, corr = (dx1/dx)^T e: all AT x_den        (:329-339)
        chunk = noise - nan_to_num(v - 0.5 corr)                                           (:347-349: the original x_t)
    so the linearisation point carries prev on the delay rows while the integrated state never does."""
    import rtc_delay_restatement as D
    import rtc_restatement as R

    r32, obs, noise, prev = tiny10["ref32"], tiny10["obs"], tiny10["noise"], tiny10["prev"]
    d, prov = 3, 14
    trace = []
    out = D.sample_actions(r32, obs, noise, 1, prev_action_chunk=prev, inference_delay=d, execute_horizon=6, mask_prefix_delay=True,
                           trace=trace)  # fmt: skip
    assert len(trace) == 1
    x_t, t, v, e, corr, x_den = trace[0]
    assert t == 1.0 and rtc.guidance_weight(1.0, 0.5) == 0.5 and torch.equal(x_t, noise)
    assert torch.equal(x_den[:, :d, :prov], prev[:, :d, :prov])
    assert torch.equal(x_den[:, d:], noise[:, d:]) and torch.equal(x_den[:, :d, prov:], noise[:, :d, prov:])
    assert torch.equal(D.linearisation_point(noise, prev, d, prov), x_den)
    # v, e and the VJP were taken at x_den, not at x_t
    ppad, cache = R.prefix_cache(r32, obs)
    one = torch.tensor(1.0)
    w = torch.from_numpy(rtc.get_prefix_weights(d, 6, 10, "exp"))
    mask = (torch.arange(32) < prov).float()
    v_den, x1_den, e_den, corr_den = R.x1_and_vjp(r32, ppad, cache, x_den, one, lambda x1: (prev - x1) * w[None, :, None] * mask)
    assert torch.equal(v, v_den) and torch.equal(e, e_den) and torch.equal(corr, corr_den)
    assert torch.equal(e_den, (prev - (x_den - one * v_den)) * w[None, :, None] * mask)
    v_at_xt = R.velocity(r32, ppad, cache, noise, one)
    assert not torch.equal(v, v_at_xt)
    # the update goes to the original x_t
    dt = torch.tensor(-1.0)
    assert torch.equal(out, noise + dt * torch.nan_to_num(v - 0.5 * corr, nan=0.0, posinf=0.0, neginf=0.0))
    assert not torch.equal(out, x_den + dt * torch.nan_to_num(v - 0.5 * corr, nan=0.0, posinf=0.0, neginf=0.0))
    assert not torch.isclose(out[:, :d, :prov], prev[:, :d, :prov]).all()  # the integrated state is not overwritten


# ------------------------------------------------------------------------------------------------ host side
def test_resolve_carries_the_flag_and_the_delay_rows():
    H, A = 10, 32
    prev = np.ones((H, 14), dtype=np.float32)
    off = rtc.resolve(prev, batch=1, action_horizon=H, action_dim=A, inference_delay=3, execute_horizon=6)
    on = rtc.resolve(prev, batch=1, action_horizon=H, action_dim=A, inference_delay=3, execute_horizon=6, mask_prefix_delay=True)
    assert off.mask_prefix_delay is False and on.mask_prefix_delay is True
    for gd in (off, on):
        assert gd.delay_rows.dtype == np.float32
        np.testing.assert_array_equal(gd.delay_rows, np.asarray([1, 1, 1] + [0] * 7, dtype=np.float32))
    np.testing.assert_array_equal(on.weights, off.weights)
    np.testing.assert_array_equal(on.prev, off.prev)
    assert not rtc.resolve(prev, batch=1, action_horizon=H, action_dim=A, mask_prefix_delay=True).delay_rows.any()  # no delay given
    assert rtc.resolve(prev, batch=1, action_horizon=H, action_dim=A, inference_delay=99, mask_prefix_delay=True).delay_rows.all()


def _cpu_model(pi05: bool):
    import dataclasses

    from tiny import tiny_cfgs

    from kai0_amd.model import PI0Pytorch
    from oracle.pi0_oracle import synthetic_batch

    pcfg, ocfg = tiny_cfgs()
    obs, actions, noise, _ = synthetic_batch(ocfg, 1, seed=0)
    return PI0Pytorch(pcfg if pi05 else dataclasses.replace(pcfg, pi05=False)), obs, actions, noise


@pytest.mark.parametrize("pi05", [True, False])
def test_model_no_longer_refuses_pi0_or_the_flag(pi05, monkeypatch):
    """pi0 with a previous chunk, and `mask_prefix_delay`, reach the engine with the flag resolved (the engine itself is HIP: a stub
    stands in for it here); bad arguments are still refused before any device work, for both variants."""
    from kai0_amd import infer

    seen = {}

    class StubEngine:
        require_hip = staticmethod(lambda device, what: None)  # (the stub stands in for a HIP-resident engine)

        def __init__(self, model, *key):
            self.key = key

        def stale(self):
            return False

        def compatible(self, *key):
            return key == self.key

        shape_matches = compatible

        def sample_actions_guided(self, images, img_masks, lang_tokens, lang_masks, noise, guidance, num_steps, state=None):
            seen.update(guidance=guidance, state=state)
            return noise

        def sample_actions(self, *a, **k):
            seen.update(guidance=None)
            return a[4]

        def replay_then_verify(self, *a, **k):
            return None

    monkeypatch.setattr(infer, "InferenceEngine", StubEngine)
    m, obs, actions, noise = _cpu_model(pi05)
    m.eval()
    m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0], inference_delay=2, mask_prefix_delay=True)
    assert seen["guidance"].mask_prefix_delay is True and seen["guidance"].delay_rows[:3].tolist() == [1.0, 1.0, 0.0]
    assert seen["state"] is not None and seen["state"].shape[0] == 1
    m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0])
    assert seen["guidance"].mask_prefix_delay is False
    for kw in (dict(prev_action_chunk=None), dict(prev_action_chunk=actions[0], enable_rtc=False)):
        m.sample_actions("cpu", obs, noise=noise, mask_prefix_delay=True, **kw)  # the flag alone does nothing
        assert seen["guidance"] is None
    with pytest.raises(ValueError):
        m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0, :-1])
    with pytest.raises(ValueError):
        m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0], prefix_attention_schedule="cosine")


@pytest.mark.parametrize("pi05", [True, False])
def test_guided_call_on_a_cpu_model_is_refused_for_its_device_only(pi05):
    """What is left of the refusals: the guided sampler is HIP launches only, so a CPU-resident model is refused — naming the device, not
    the model family or the flag — after the arguments were validated and before an engine is built."""
    m, obs, actions, noise = _cpu_model(pi05)
    m.eval()
    for flag in (False, True):
        with pytest.raises(NotImplementedError, match="HIP engine only.*cpu"):
            m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0], mask_prefix_delay=flag)
        with pytest.raises(ValueError):
            m.sample_actions("cpu", obs, noise=noise, prev_action_chunk=actions[0, :-1], mask_prefix_delay=flag)
    assert m._engine is None


def test_policy_sends_the_flag_only_from_its_sample_kwargs():
    """The reference's Policy never sends `mask_prefix_delay` (policy.py:84-90 hands on three keys): a request cannot switch it on, a
    deployment can, through the sample kwargs."""
    from test_rtc_cpu import _request, _StubModel

    from kai0_amd.policy import Policy

    chunk = np.zeros((10, 14), dtype=np.float32)
    stub = _StubModel()
    Policy(stub, pytorch_device="cpu", device_resize=False).infer(_request(prev_action_chunk=chunk.tolist(), inference_delay=2))
    assert "mask_prefix_delay" not in stub.calls[0]
    stub = _StubModel()
    pol = Policy(stub, pytorch_device="cpu", device_resize=False, sample_kwargs={"mask_prefix_delay": True})
    pol.infer(_request(prev_action_chunk=chunk.tolist(), inference_delay=2))
    pol.infer(_request())
    assert stub.calls[0]["mask_prefix_delay"] is True and stub.calls[0]["inference_delay"] == 2
    assert stub.calls[1] == {"mask_prefix_delay": True}  # without a previous chunk the model ignores it


# ------------------------------------------------------------------------------------------------ header / binding
def test_overwrite_seam_is_declared_and_bound():
    from kai0_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "kai0hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int kai0_rtc_overwrite(const float* x, const float* prev, const float* row_mask, int provided, float* out, int64_t rows, "
            "int Hs, int A, kai0_stream_t stream);") in flat  # fmt: skip
    assert "pi0_rtc.py:322-327" in header
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib._PROTOS["kai0_rtc_overwrite"] == [p, p, p, i, p, i64, i, i, p]
    assert "kai0_rtc_overwrite" in set(_lib.EXPORTED_SYMBOLS) and _lib.ABI_VERSION == 4
    assert callable(ops.rtc_overwrite)
