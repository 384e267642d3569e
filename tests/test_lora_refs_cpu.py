"""tests/lora_refs.py held against itself on the CPU: (a) the f32 emulation of kai0_lora_down / kai0_lora_wgrad (f32 matmul, the
header's rounding points, slices summed in slice order) stays inside the derived per-element bound at the shapes
tests/test_lora_kernels_gpu.py uses, and (b) the defects that file exists to catch — a dropped contraction tail, a slice counted
twice, the scale applied after the rounding, a transposed store — are rejected when planted into the emulation.  No HIP library,
no GPU."""

import pytest
import torch

import lora_refs as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _down(M, K, R_):
    return R.randn(M, K, seed=1), R.randn(R_, K, seed=2, scale=0.05)


def _wgrad(M, R_, C):
    return R.randn(M, R_, seed=3), R.randn(M, C, seed=4)


@pytest.mark.parametrize("k_chunk", [None, 256])
@pytest.mark.parametrize("M,K,R_", [(1, 8, 16), (65, 264, 32), (257, 2056, 64), (65, 16384, 16)])
def test_down_emulation_stays_within_the_bound(M, K, R_, k_chunk):
    x, a = _down(M, K, R_)
    ref, bound = R.down_reference(x, a)
    w = R.assert_within(R.down_emulate(x, a, k_chunk), ref, bound, f"down {M}x{K}x{R_}")
    print(f"down {M}x{K}x{R_} chunk {k_chunk}: worst err / bound {w:.3f}")
    if K == 264:  # the one bf16 rounding dominates: the bound must be nearly reached, or it is loose
        assert w > 0.9, f"worst err / bound {w:.3f}"


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("M,R_,C,slice_rows", [(1, 16, 8, None), (33, 64, 136, None), (1000, 16, 264, 64), (4099, 64, 136, 1088)])
def test_wgrad_emulation_stays_within_the_bound(M, R_, C, slice_rows, scale, out_f32):
    p, q = _wgrad(M, R_, C)
    for tr in (False, True):
        ref, bound = R.wgrad_reference(p, q, scale, out_f32, tr)
        out = R.wgrad_emulate(p, q, scale, out_f32, tr, slice_rows)
        assert out.dtype == (F32 if out_f32 else BF16) and tuple(out.shape) == ((C, R_) if tr else (R_, C))
        w = R.assert_within(out, ref, bound, f"wgrad {M}x{R_}x{C} scale {scale} f32 {out_f32} transposed {tr}")
    print(f"wgrad {M}x{R_}x{C} scale {scale} f32 {out_f32}: worst err / bound {w:.3f}")
    if M == 33 and not out_f32:
        assert w > 0.9, f"worst err / bound {w:.3f}"


def test_f32_wgrad_bound_has_no_bf16_term():
    """The f32 output's bound is the accumulation term plus one f32 ulp of the result: (M + 1) 2^-23 |P|^T |Q| covers it."""
    p, q = _wgrad(1000, 16, 264)
    _, bound = R.wgrad_reference(p, q, 1.0, True)
    t = p.to(F64).abs().T @ q.to(F64).abs()
    assert bool((bound <= 1001 * 2.0**-23 * t + 2.0**-125).all())


def test_planted_defects_are_rejected():
    x, a = _down(65, 264, 32)
    ref, bound = R.down_reference(x, a)
    with pytest.raises(AssertionError):  # the last 8 contraction elements never staged
        R.assert_within(R.down_emulate(x[:, :256], a[:, :256]), ref, bound, "tail")
    with pytest.raises(AssertionError):  # adapter rows 16 .. 31 swapped with 0 .. 15
        R.assert_within(R.down_emulate(x, a.roll(16, 0)), ref, bound, "rows")
    p, q = _wgrad(1000, 16, 264)
    ref, bound = R.wgrad_reference(p, q, 0.3)
    twice = torch.cat([p, p[-40:]]), torch.cat([q, q[-40:]])  # the ragged last slice added twice
    with pytest.raises(AssertionError):
        R.assert_within(R.wgrad_emulate(*twice, 0.3), ref, bound, "slice twice")
    with pytest.raises(AssertionError):  # rows past M staged as data instead of zeros
        R.assert_within(R.wgrad_emulate(p[:960], q[:960], 0.3), ref, bound, "short")
    late = (R.wgrad_emulate(p, q, 1.0).float() * 0.3).to(BF16)  # rounded to bf16 BEFORE the scale: a second rounding
    with pytest.raises(AssertionError):
        R.assert_within(late, ref, bound, "scale after rounding")
    sq_p, sq_q = _wgrad(64, 16, 16)
    ref, bound = R.wgrad_reference(sq_p, sq_q, 1.0, False, True)
    with pytest.raises(AssertionError):  # direct store where the transposed one was asked for (square: same shape)
        R.assert_within(R.wgrad_emulate(sq_p, sq_q, 1.0, False, False), ref, bound, "orientation")


def test_guarded_window_detects_stray_writes():
    g = R.Guarded(3, 16, 32, BF16, "cpu")
    g.t.copy_(torch.ones(3, 16))
    g.check("clean")
    g.buf[R.GUARD + 16] = 1.0  # first padding element of row 0
    with pytest.raises(AssertionError):
        g.check("padding")
    g = R.Guarded(3, 16, 32, BF16, "cpu")
    g.t[:2].fill_(1.0)
    with pytest.raises(AssertionError):
        g.check("unwritten row")
