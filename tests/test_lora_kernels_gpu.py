"""kai0_lora_down / kai0_lora_wgrad (csrc/lora.hip) against the float64 references and derived per-element bounds of
tests/lora_refs.py.  Every output sits in a padded window of a sentinel-filled buffer (lora_refs.Guarded): the guard bands in front
and behind AND the padding between the rows must survive, and every element of the window must be written.

Shapes are a product of small sets around the kernels' own edges, not the workload: lora_down's block is 64 rows (M around it, and
more than one block), its staged chunk 256 contraction elements (K below, across and far beyond it, none a multiple of 32 except
via the 8-element granularity), every supported R; lora_wgrad's stage is 64 rows and its slices multiples of that (M = 1 and 31:
one short slice; 33, 1000, 4099: several slices with a ragged last one), its column tile 128 (C below, across one and two tiles),
R one and four MFMA tiles, both output dtypes and orientations, scale 1 and 0.5, all leading dimensions padded."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lora_refs as R  # noqa: E402
from lora_refs import BF16, F32  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from kai0_amd import _lib

    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(t, ld):
    """A copy of t [rows, cols] with row stride ld (the padding holds NaN: reading it poisons the result)."""
    rows, cols = t.shape
    buf = torch.full((rows, ld), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :cols] = t
    return buf


_DOWN_REF = {}


def _down_case(M, K, Rr):
    """Inputs on the device and (ref, bound), computed once per shape."""
    key = (M, K, Rr)
    if key not in _DOWN_REF:
        x, a = R.randn(M, K, seed=11, device=DEV), R.randn(Rr, K, seed=12, scale=0.05, device=DEV)
        _DOWN_REF[key] = (x, a, *R.down_reference(x, a))
    return _DOWN_REF[key]


def _run_down(M, K, Rr):
    x, a, ref, bound = _down_case(M, K, Rr)
    xs, as_ = _padded(x, K + 8), _padded(a, K + 8)
    out = R.Guarded(M, Rr, Rr + 16, BF16, DEV)
    _lib().call("kai0_lora_down", xs.data_ptr(), K + 8, as_.data_ptr(), K + 8, out.ptr(), Rr + 16, M, Rr, K, _stream())
    torch.cuda.synchronize()
    out.check(f"lora_down {M}x{K}x{Rr}")
    return R.assert_within(out.t, ref, bound, f"lora_down {M}x{K}x{Rr}")


@pytest.mark.parametrize("Rr", [16, 32, 48, 64])
@pytest.mark.parametrize("K", [8, 72, 264, 2056])
def test_lora_down(K, Rr):
    for M in (1, 63, 64, 65, 257):
        w = _run_down(M, K, Rr)
        print(f"lora_down M={M} K={K} R={Rr}: worst err / bound {w:.3f}")


def test_lora_down_long_contraction():
    w = _run_down(65, 16384, 16)
    print(f"lora_down M=65 K=16384 R=16: worst err / bound {w:.3f}")


def test_lora_down_rejects_what_it_does_not_support():
    lib = _lib()
    x = torch.zeros(64, 64, dtype=BF16, device=DEV)
    t = torch.zeros(64, 64, dtype=BF16, device=DEV)
    for M, Rr, K, ld in [(64, 8, 64, 64), (64, 24, 64, 64), (64, 16, 12, 64), (64, 16, 64, 60), (64, 16, 64, 4)]:
        with pytest.raises(lib.Kai0HipError):
            lib.call("kai0_lora_down", x.data_ptr(), ld, x.data_ptr(), ld, t.data_ptr(), 64, M, Rr, K, _stream())
    with pytest.raises(lib.Kai0HipError):  # X not 16-byte aligned
        lib.call("kai0_lora_down", x.data_ptr() + 2, 64, x.data_ptr(), 64, t.data_ptr(), 64, 8, 16, 32, _stream())


_WGRAD_IN = {}


def _wgrad_inputs(M, Rr, C):
    key = (M, Rr, C)
    if key not in _WGRAD_IN:
        _WGRAD_IN[key] = (R.randn(M, Rr, seed=13, device=DEV), R.randn(M, C, seed=14, device=DEV))
    return _WGRAD_IN[key]


def _run_wgrad(M, Rr, C, scale, out_f32, transposed, ws_fill=float("nan")):
    lib = _lib()
    p, q = _wgrad_inputs(M, Rr, C)
    ps, qs = _padded(p, Rr + 8), _padded(q, C + 16)
    rows, cols = (C, Rr) if transposed else (Rr, C)
    out = R.Guarded(rows, cols, cols + 8, F32 if out_f32 else BF16, DEV)
    nbytes = lib.load().kai0_lora_wgrad_workspace_bytes(M, Rr, C)
    assert nbytes >= Rr * C * 4 and nbytes % (Rr * C * 4) == 0
    ws = R.Guarded(1, nbytes // 4, nbytes // 4, F32, DEV)  # the workspace is guarded too: exactly the advertised size
    ws.t.fill_(ws_fill)
    lib.call("kai0_lora_wgrad", ps.data_ptr(), Rr + 8, qs.data_ptr(), C + 16, out.ptr(), cols + 8, M, Rr, C, scale, int(transposed),
             int(out_f32), ws.ptr(), nbytes, _stream())  # fmt: skip
    torch.cuda.synchronize()
    what = f"lora_wgrad {M}x{Rr}x{C} scale {scale} f32 {out_f32} transposed {transposed}"
    out.check(what)
    ws.check(what + " (workspace)")  # every partial element was written as well, none outside
    return out.t.clone(), what


@pytest.mark.parametrize("C", [8, 136, 264])
@pytest.mark.parametrize("Rr", [16, 64])
@pytest.mark.parametrize("M", [1, 31, 33, 1000, 4099])
def test_lora_wgrad(M, Rr, C):
    p, q = _wgrad_inputs(M, Rr, C)
    for scale in (1.0, 0.5):
        for out_f32 in (False, True):
            for transposed in (False, True):
                ref, bound = R.wgrad_reference(p, q, scale, out_f32, transposed)
                out, what = _run_wgrad(M, Rr, C, scale, out_f32, transposed)
                w = R.assert_within(out, ref, bound, what)
                again, _ = _run_wgrad(M, Rr, C, scale, out_f32, transposed, ws_fill=7.0)  # other stale workspace contents
                assert torch.equal(out, again), f"{what}: two runs differ"
    print(f"lora_wgrad M={M} R={Rr} C={C}: worst err / bound {w:.3f} (last form)")


def test_lora_wgrad_rank_8():
    """R = 8 (half an MFMA tile: the project's test variant): the upper half of the tile is staged as zeros and never stored."""
    p, q = _wgrad_inputs(300, 8, 136)
    for transposed in (False, True):
        ref, bound = R.wgrad_reference(p, q, 2.0, False, transposed)
        out, what = _run_wgrad(300, 8, 136, 2.0, False, transposed)
        R.assert_within(out, ref, bound, what)


def test_lora_wgrad_rejects_a_short_workspace():
    lib = _lib()
    p, q = _wgrad_inputs(1000, 16, 136)
    g = torch.zeros(16, 136, dtype=BF16, device=DEV)
    need = lib.load().kai0_lora_wgrad_workspace_bytes(1000, 16, 136)
    ws = torch.zeros(need // 4, dtype=F32, device=DEV)
    with pytest.raises(lib.Kai0HipError):
        lib.call("kai0_lora_wgrad", p.data_ptr(), 16, q.data_ptr(), 136, g.data_ptr(), 136, 1000, 16, 136, 1.0, 0, 0, ws.data_ptr(), need - 4,
                 _stream())  # fmt: skip
    with pytest.raises(lib.Kai0HipError):  # C not a multiple of 8
        lib.call("kai0_lora_wgrad", p.data_ptr(), 16, q.data_ptr(), 136, g.data_ptr(), 136, 1000, 16, 132, 1.0, 0, 0, ws.data_ptr(), need,
                 _stream())  # fmt: skip
