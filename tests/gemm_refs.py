"""Float64 references and per-element error bounds for kai0_gemm_bf16 (csrc/gemm_bf16.hip), after the epilogue order of
include/kai0hip.h.  A plain helper module like tests/streaming_refs.py: nothing here touches the HIP library, everything runs on
whichever device its inputs live on.

One formula.  `accumulate` and `epilogue` state C = op(A) op(B) and the linear epilogue ONCE, for either working dtype:

  dt = float64  the reference.  No intermediate rounding (a reference that rounded inside would sit on the other side of a rounding
                boundary from a correct kernel now and then and be off by a whole bf16 ulp there); the header's rounding points are
                accounted for in the bound instead, which `epilogue` builds alongside the value.
  dt = float32  the emulation tests/test_gemm_refs_cpu.py holds against the bound: an f32 matmul with the header's bf16 rounding
                points.  The kernels are never used to choose a constant.

The epilogue (kai0hip.h), on the f32 accumulator v:
  v += bias[col];  v = bf16(v);  if scale != 1: v = bf16(v * scale);  if gate: v = bf16(v * gate[row / gate_rpb][col]);
  if residual: v = bf16(v + residual[row][col]);  if accumulate: v = v + C_old;  C = v, rounded to bf16 once more unless out_f32.
With out_f32 none of the bf16 roundings is applied: every step is one f32 operation.

The bound, per element, derived and not measured.  Write U32 = 2^-23 (one f32 ulp, relative: twice the rounding error of one f32
operation), UBF = 2^-8 (the rounding error of one round-to-nearest bf16 rounding, relative: half of the 2^-7 ulp), T = |A| |B|
evaluated in f64, and carry (x, e) = (exact value, bound on |computed - exact|) through the chain:

  accumulation   x = sum_k a b, e = K * U32 * T.  The products of two bf16 values are exact in f32.  Any summation of K f32 terms
                 into one f32 value, in any order and any grouping, is off by at most (K - 1) * 2^-24 * sum|terms| * (1 + O(K 2^-24))
                 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); K * U32 * T is twice that, which leaves
                 the same again for an MFMA that aligns the addends of one instruction before it adds them.  Independent of the
                 order, so it holds for every K loop, for split-K (slices summed in f32 by the reduction: still K terms in some
                 grouping) and for empty slices.  MI355X_MICROARCH.md gives no looser figure for the bf16 MFMA (it states exact
                 f32 behaviour for the f32-input MFMA only), so none is used.
  f32 add / mul  (x, e) -> (x', e' + U32 * |x'|), e' the incoming error carried through the operation: e for an add,
                 |factor| * e for a multiply by an exactly known factor (scale, gate).  One such term per f32 operation after the
                 accumulation: bias add, scale, gate, residual add, accumulate.
  bf16 rounding  (x, e) -> (x, e + UBF * (|x| + e)): the rounded number is the computed one, at most |x| + e in magnitude.
  store          bf16 output after `accumulate`: one more bf16 rounding.  Otherwise nothing: the chain ends on a bf16 value (or,
                 with out_f32, on the f32 value that is stored).
  floor          + 2^-126 (the smallest normal number: below it a result may lose bits).

`assert_within` holds EVERY element to that bound; no share of the elements is exempt.
"""

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U32 = 2.0**-23
UBF = 2.0**-8
TINY = 2.0**-126
SENTINEL = -24576.0  # exactly representable in bf16 and f32, far from every result


def view(storage, rows, cols, ld, *, outer=1, inner=1, s1=0, s2=0, offset=0):
    """The [outer, inner, rows, cols] window of a stored operand: entry (z1, z2) starts at offset + z1 * s1 + z2 * s2 elements, its
    rows are `ld` apart (kai0hip.h "Batching")."""
    flat = storage.reshape(-1)
    return flat.as_strided((outer, inner, rows, cols), (s1, s2, ld, 1), flat.storage_offset() + offset)


def operands(a_store, b_store, lay, M, N, K, lda, ldb, *, outer=1, inner=1, sA=(0, 0), sB=(0, 0)):
    """Logical A [.., M, K] and B [.., K, N] of layout `lay` in NT / NN / TN / TT: first letter N = A stored [M][K] (a_kc = 1), T = A
    stored [K][M]; second letter T = B stored [N][K] (b_kc = 1, an nn.Linear weight), N = B stored [K][N]."""
    kw = dict(outer=outer, inner=inner)
    a = view(a_store, M, K, lda, s1=sA[0], s2=sA[1], **kw) if lay[0] == "N" else view(a_store, K, M, lda, s1=sA[0], s2=sA[1], **kw).transpose(-1, -2)
    b = view(b_store, N, K, ldb, s1=sB[0], s2=sB[1], **kw).transpose(-1, -2) if lay[1] == "T" else view(b_store, K, N, ldb, s1=sB[0], s2=sB[1], **kw)
    return a, b


def layout_flags(lay):
    return {"a_kc": lay[0] == "N", "b_kc": lay[1] == "T"}


def accumulate(a, b, dt, k_chunk=None):
    """op(A) op(B) in `dt`; with k_chunk, the sum over split-K slices [s * k_chunk, (s + 1) * k_chunk) in slice order (the reduction's)."""
    K = a.shape[-1]
    if k_chunk is None or k_chunk >= K:
        return a.to(dt) @ b.to(dt)
    acc = None
    for k0 in range(0, K, k_chunk):
        part = a[..., k0 : k0 + k_chunk].to(dt) @ b[..., k0 : k0 + k_chunk, :].to(dt)
        acc = part if acc is None else acc + part
    return acc


class Chain:
    """(value, err) carried through the epilogue: the float64 reference with its bound (track = True) or the f32 emulation."""

    def __init__(self, value, err=None):
        self.v, self.e = value, err

    def f32_op(self, value, carried):
        self.v = value
        if self.e is not None:
            self.e = carried + U32 * value.abs()

    def add(self, other):
        self.f32_op(self.v + other.to(self.v.dtype), self.e)

    def mul(self, factor):
        f = factor.to(self.v.dtype) if torch.is_tensor(factor) else factor
        self.f32_op(self.v * f, None if self.e is None else self.e * (f.abs() if torch.is_tensor(f) else abs(f)))

    def round_bf16(self):
        if self.e is not None:
            self.e = self.e + UBF * (self.v.abs() + self.e)
        else:
            self.v = self.v.to(BF16).to(self.v.dtype)


def epilogue(acc, err=None, *, bias=None, scale=1.0, gate=None, residual=None, c_old=None, out_f32=False):
    """The linear epilogue of kai0hip.h on an accumulator.  err = None: the emulation (acc is f32; returns the stored tensor, bf16 or
    f32).  err given: the reference (acc is f64; returns (ref f64, bound f64)).  bias [N], gate / residual / c_old broadcastable to
    acc (the caller expands gate rows by gate_rpb)."""
    c = Chain(acc, err)
    rnd = (lambda: None) if out_f32 else c.round_bf16
    if bias is not None:
        c.add(bias)
    rnd()
    if scale != 1.0:
        c.mul(float(torch.tensor(scale, dtype=F32)))
        rnd()
    if gate is not None:
        c.mul(gate)
        rnd()
    if residual is not None:
        c.add(residual)
        rnd()
    if c_old is not None:
        c.add(c_old)
    if err is None:
        return c.v.to(F32 if out_f32 else BF16)
    if c_old is not None:
        rnd()  # the store rounds once more only after the accumulate add: every other chain ends on a bf16 value already
    return c.v, c.e + TINY


def reference(a, b, **epi):
    """(ref, bound), both float64, for logical operands a [.., M, K] and b [.., K, N] (bf16 values) and the epilogue of `epilogue`."""
    a64, b64 = a.to(F64), b.to(F64)
    T = a64.abs() @ b64.abs()
    return epilogue(a64 @ b64, a.shape[-1] * U32 * T, **epi)


def emulate(a, b, k_chunk=None, **epi):
    """The f32 evaluation with the header's rounding points, as stored (bf16, or f32 with out_f32)."""
    return epilogue(accumulate(a, b, F32, k_chunk), None, **epi)


def worst(out, ref, bound):
    """(worst err / bound, index of that element, number of elements outside the bound).  A non-finite output counts as outside."""
    err = (out.to(F64) - ref).abs()
    ratio = err / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    bad = int((~(err <= bound)).sum())  # (NaN compares False: outside)
    flat = int(ratio.reshape(-1).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
    return float(ratio.reshape(-1)[flat]), idx, bad


def assert_within(out, ref, bound, what=""):
    """Every element of `out` within `bound` of `ref` (same shape; leading dimensions = batch, last two = row, col).  Returns the
    worst err / bound."""
    assert tuple(out.shape) == tuple(ref.shape) == tuple(bound.shape), f"{what}: shapes {tuple(out.shape)} / {tuple(ref.shape)}"
    w, idx, bad = worst(out, ref, bound)
    if bad:
        batch, (row, col) = idx[:-2], idx[-2:]
        raise AssertionError(
            f"{what}: {bad} of {out.numel()} elements outside the bound; worst err / bound {w:.3g} at batch {batch} row {row} col {col}: "
            f"got {float(out[idx]):.9g}, reference {float(ref[idx]):.9g}, bound {float(bound[idx]):.3g}")
    return w
