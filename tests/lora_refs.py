"""Float64 references and per-element error bounds for the two LoRA kernels (csrc/lora.hip; include/kai0hip.h kai0_lora_down /
kai0_lora_wgrad).  A plain helper module like tests/gemm_refs.py, whose rules it applies unchanged (the derivation is in that module's
docstring): nothing here touches the HIP library.

  kai0_lora_down    T = bf16( X A^T ): f32 accumulation over K, one bf16 rounding.
  kai0_lora_wgrad   G = bf16 or f32( (sum_m P[m][r] Q[m][c]) * scale ): f32 accumulation over M (slices of M summed in f32 in slice
                    order: still M terms in some grouping), ONE f32 multiply by scale, then the rounding of the store (none for f32).

The bound per element, with U32 = 2^-23, UBF = 2^-8 and (x, e) = (exact value, bound on |computed - exact|):
  accumulation   e = L * U32 * (|P|^T |Q|), L the contraction length (K for down, M for wgrad), independent of order and grouping
  f32 multiply   (x, e) -> (x s, |s| e + U32 |x s|)     — applied for every scale, 1 included (exact there: the term only loosens
                                                           the bound by one f32 ulp and keeps one formula)
  bf16 rounding  (x, e) -> (x, e + UBF (|x| + e))
  floor          + 2^-126
No element is exempt and no constant is fitted to the kernels; tests/test_lora_refs_cpu.py holds an f32 emulation with the same
rounding points to it."""

import torch

import gemm_refs as G

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENTINEL = G.SENTINEL
GUARD = 64  # sentinel elements on both sides of every output


def randn(*shape, seed, scale=1.0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16).to(device)


def _chain(acc, err, scale, out_f32):
    c = G.Chain(acc, err)
    if scale is not None:
        c.mul(float(torch.tensor(scale, dtype=F32)))
    if not out_f32:
        c.round_bf16()
    return c


def down_reference(x, a):
    """(ref, bound), float64 [M, R], for x [M, K] and a [R, K] (bf16 values)."""
    x64, a64 = x.to(F64), a.to(F64)
    c = _chain(x64 @ a64.T, x.shape[1] * G.U32 * (x64.abs() @ a64.abs().T), None, False)
    return c.v, c.e + G.TINY


def down_emulate(x, a, k_chunk=None):
    """f32 products summed in f32 (optionally chunk by chunk), one bf16 rounding: what the kernel stores."""
    return _chain(G.accumulate(x, a.T, F32, k_chunk), None, None, False).v.to(BF16)


def wgrad_reference(p, q, scale=1.0, out_f32=False, transposed=False):
    """(ref, bound), float64 [R, C] (or [C, R] transposed), for p [M, R] and q [M, C] (bf16 values)."""
    p64, q64 = p.to(F64), q.to(F64)
    c = _chain(p64.T @ q64, p.shape[0] * G.U32 * (p64.abs().T @ q64.abs()), scale, out_f32)
    v, e = c.v, c.e + G.TINY
    return (v.T, e.T) if transposed else (v, e)


def wgrad_emulate(p, q, scale=1.0, out_f32=False, transposed=False, slice_rows=None):
    """Slices of M summed in f32 in slice order, one f32 multiply, the store's rounding."""
    c = _chain(G.accumulate(p.T, q, F32, slice_rows), None, scale, out_f32)
    v = c.v.to(F32 if out_f32 else BF16)
    return v.T if transposed else v


assert_within = G.assert_within


class Guarded:
    """An [rows, cols] window with row stride `ld` inside a buffer filled with SENTINEL: GUARD elements in front and behind, and the
    ld - cols elements between the rows, must all survive the launch; the window itself starts as NaN and must be fully written."""

    def __init__(self, rows, cols, ld, dtype, device):
        n = (rows - 1) * ld + cols if rows else 0
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=device)
        self.t = self.buf.as_strided((rows, cols), (ld, 1), GUARD)
        self.t.fill_(float("nan"))
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask.as_strided((rows, cols), (ld, 1), GUARD).fill_(False)

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def check(self, what):
        assert bool((self.buf[self.mask] == SENTINEL).all()), f"{what}: wrote outside its output"
        left = int(torch.isnan(self.t).sum())
        assert left == 0, f"{what}: {left} of {self.t.numel()} elements never written"
