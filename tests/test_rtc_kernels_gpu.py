"""kai0_rtc_error / kai0_rtc_update (csrc/rtc.hip) against their torch formulas, bit for bit: every product and sum rounds to f32 on
its own, so torch's element-wise f32 ops on the CPU restate them exactly.  Shapes: one vector per lane with a scalar tail
(3 x 7 x 32), more than one block (1 x 50 x 32 = 1600 elements), views that start 4 / 8 / 12 bytes past a 16-byte boundary (the
all-scalar fallback when the buffers disagree, head + body + tail when they agree)."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

F32 = torch.float32
SHAPES = [(1, 50, 32), (2, 10, 32), (3, 7, 32)]
T, G, DT = 0.7000000476837158, 2.1666667461395264, -0.10000000149011612  # f32 values, as the engine passes them


def dev():
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _on_gpu(t, offset=0):
    """`t` on the GPU as a contiguous view that starts `offset` f32 elements past an allocation's (256-byte aligned) base."""
    buf = torch.empty(t.numel() + 8, dtype=F32, device=dev())
    v = buf[offset : offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _same(a, b):
    """bit-equal where finite, NaN where NaN (payloads are not compared)"""
    a, b = a.cpu(), b.cpu()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


def error_ref(x, v, prev, w, provided, t):
    tt = torch.tensor(t, dtype=F32)
    mask = (torch.arange(x.shape[-1]) < provided).to(F32)
    return ((prev - (x - tt * v)) * w[None, :, None]) * mask


def update_ref(x, v, err, jte, t, g, dt):
    tt, gg, dd = (torch.tensor(s, dtype=F32) for s in (t, g, dt))
    vn = torch.nan_to_num(v - gg * (err - tt * jte), nan=0.0, posinf=0.0, neginf=0.0)
    return x + dd * vn


def _weights(Hs):
    w = torch.rand(Hs, generator=torch.Generator().manual_seed(5))
    w[Hs // 2 :] = 0.0  # rows past the execute horizon
    w[0] = 1.0
    return w


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("provided", [0, 14, 32])
def test_rtc_error_matches_torch_bitwise(shape, provided):
    from kai0_amd import ops

    x, v, prev = _rand(shape, 1), _rand(shape, 2, 3.0), _rand(shape, 3)
    v.view(-1)[[3, 17, 40]] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    w = _weights(shape[1])
    got = ops.rtc_error(_on_gpu(x), _on_gpu(v), _on_gpu(prev), w.to(dev()), provided, T)
    assert _same(got, error_ref(x, v, prev, w, provided, T))
    if provided == 0:
        assert not torch.nan_to_num(got, nan=0.0).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_rtc_update_matches_torch_bitwise(shape):
    from kai0_amd import ops

    x, v, err, jte = _rand(shape, 1), _rand(shape, 2, 3.0), _rand(shape, 3), _rand(shape, 4, 5.0)
    v.view(-1)[[3, 17, 40]] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    jte.view(-1)[[5, 17, 41, 60]] = torch.tensor([float("nan"), float("-inf"), float("inf"), 3e38])  # (3e38 * g overflows: -> 0)
    xg = _on_gpu(x)
    ops.rtc_update_(xg, _on_gpu(v), _on_gpu(err), _on_gpu(jte), T, G, DT)
    ref = update_ref(x, v, err, jte, T, G, DT)
    assert torch.isfinite(ref).all() and torch.equal(xg.cpu(), ref)
    assert torch.equal(xg.cpu().view(-1)[[3, 17, 41, 60]], x.view(-1)[[3, 17, 41, 60]])  # a non-finite velocity moves nothing


@pytest.mark.parametrize("offsets", [(1, 1, 1, 1), (3, 3, 3, 3), (0, 1, 2, 3), (2, 2, 0, 2)])
def test_rtc_seams_on_unaligned_views(offsets):
    from kai0_amd import ops

    shape = (3, 7, 32)
    x, v, prev, jte = _rand(shape, 1), _rand(shape, 2), _rand(shape, 3), _rand(shape, 4)
    w = _weights(shape[1])
    o = offsets
    out = _on_gpu(torch.zeros(shape), o[3])
    ops.rtc_error(_on_gpu(x, o[0]), _on_gpu(v, o[1]), _on_gpu(prev, o[2]), w.to(dev()), 14, T, out=out)
    err = error_ref(x, v, prev, w, 14, T)
    assert torch.equal(out.cpu(), err)
    xg = _on_gpu(x, o[0])
    ops.rtc_update_(xg, _on_gpu(v, o[1]), _on_gpu(err, o[2]), _on_gpu(jte, o[3]), T, G, DT)
    assert torch.equal(xg.cpu(), update_ref(x, v, err, jte, T, G, DT))


@pytest.mark.parametrize("shape", SHAPES)
def test_rtc_update_without_correction_is_the_euler_step(shape):
    from kai0_amd import ops

    x, v = _rand(shape, 1), _rand(shape, 2, 3.0)
    zero = torch.zeros(shape, device=dev())
    a, b = _on_gpu(x), _on_gpu(x)
    ops.rtc_update_(a, _on_gpu(v), zero, zero, T, G, DT)
    ops.euler_step_(b, _on_gpu(v), DT)
    assert torch.equal(a, b)
