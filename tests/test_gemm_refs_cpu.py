"""tests/gemm_refs.py held against itself on the CPU: (a) the f32 emulation of kai0_gemm_bf16 (f32 matmul, the header's bf16 rounding
points) stays inside the derived per-element bound for every reference / epilogue form tests/test_gemm_big_tile_gpu.py uses, and
(b) the defects that file exists to catch — a mis-staged K tail, a shifted ragged block, a wrong batch stride, a stale split-K
slice — are rejected when planted into the emulation.  No HIP library, no GPU."""

import pytest
import torch

import gemm_refs as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SHAPES = [(200, 136, 264), (264, 520, 1000), (136, 264, 4104)]
OUTER, INNER = 2, 3  # a small two-level batch: the bound is per element, more entries add nothing


def _rnd(*shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _case(M, N, K, form):
    """Logical operands and the epilogue keywords of one form; the inputs of the GPU file: A ~ N(0,1), B ~ 0.05 N(0,1)."""
    a, b = _rnd(OUTER, INNER, M, K, seed=1), _rnd(OUTER, INNER, K, N, seed=2, scale=0.05)
    bias, gate = _rnd(N, seed=3), _rnd(M // 8, N, seed=4).repeat_interleave(8, 0)
    res, c_old = _rnd(OUTER, INNER, M, N, seed=5), _rnd(OUTER, INNER, M, N, seed=6)
    epi = {
        "plain": {},
        "bias": dict(bias=bias),
        "bias_f32": dict(bias=_rnd(N, seed=3, dtype=F32)),
        "residual": dict(residual=res),
        "gate": dict(gate=gate),
        "scale": dict(scale=0.0625),
        "scale_odd": dict(scale=0.3),
        "accumulate": dict(c_old=c_old),
        "accumulate_bias_residual": dict(c_old=c_old, bias=bias, residual=res),
        "bias_gate_residual": dict(bias=bias, gate=gate, residual=res),
        "out_f32": dict(out_f32=True),
        "out_f32_accumulate": dict(out_f32=True, c_old=c_old.float() * 3.0),
        "out_f32_bias_residual": dict(out_f32=True, bias=bias, residual=res),
    }[form]
    return a, b, epi


FORMS = ["plain", "bias", "bias_f32", "residual", "gate", "scale", "scale_odd", "accumulate", "accumulate_bias_residual", "bias_gate_residual",
         "out_f32", "out_f32_accumulate", "out_f32_bias_residual"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_emulation_stays_within_the_bound(M, N, K, form):
    a, b, epi = _case(M, N, K, form)
    ref, bound = R.reference(a, b, **epi)
    w = R.assert_within(R.emulate(a, b, **epi), ref, bound, f"{form} {M}x{N}x{K}")
    print(f"{form} {M}x{N}x{K}: worst err / bound {w:.3f}")
    if K == 264 and form in ("plain", "bias_gate_residual"):  # one bf16 rounding dominates: the bound must be nearly reached, or it is loose
        assert w > 0.9, f"{form}: worst err / bound {w:.3f}"


@pytest.mark.parametrize("k_chunk", [64, 128, 320])
@pytest.mark.parametrize("form", ["plain", "accumulate_bias_residual", "out_f32"])
def test_split_k_emulation_stays_within_the_same_bound(form, k_chunk):
    """The bound does not depend on the summation order: slices summed in f32 fit it unchanged."""
    a, b, epi = _case(200, 136, 264, form)
    ref, bound = R.reference(a, b, **epi)
    R.assert_within(R.emulate(a, b, k_chunk=k_chunk, **epi), ref, bound, f"split {form} chunk {k_chunk}")


def test_views_follow_two_level_batch_strides():
    """`view` / `operands` against plain indexing, on padded strides with s1 != inner * s2."""
    M, N, K, lda, ldb = 16, 8, 24, 32, 40
    s2a, s2b = K * lda + 8, K * ldb + 16  # (room for either layout: [K][M] / [K][N] rows as well)
    s1a, s1b = INNER * s2a + 24, INNER * s2b + 8
    sa, sb = _rnd(OUTER * s1a, seed=1), _rnd(OUTER * s1b, seed=2)
    a, b = R.operands(sa, sb, "NT", M, N, K, lda, ldb, outer=OUTER, inner=INNER, sA=(s1a, s2a), sB=(s1b, s2b))
    assert a.shape == (OUTER, INNER, M, K) and b.shape == (OUTER, INNER, K, N)
    for z1, z2, r, c in [(0, 0, 0, 0), (1, 2, 15, 23), (1, 0, 3, 7), (0, 2, 9, 1)]:
        assert a[z1, z2, r, c] == sa[z1 * s1a + z2 * s2a + r * lda + c]
        assert b[z1, z2, c, r % N] == sb[z1 * s1b + z2 * s2b + (r % N) * ldb + c]
    at, bn = R.operands(sa, sb, "TN", M, N, K, lda, ldb, outer=OUTER, inner=INNER, sA=(s1a, s2a), sB=(s1b, s2b))
    assert at[1, 2, 5, 7] == sa[s1a + 2 * s2a + 7 * lda + 5] and bn[1, 2, 7, 5] == sb[s1b + 2 * s2b + 7 * ldb + 5]


# ------------------------------------------------------------------------------------------------ planted defects
def _plain(K=264):
    a, b, _ = _case(200, 136, K, "plain")
    return a, b, R.reference(a, b)


def _rejected(out, ref, bound, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        R.assert_within(out, ref, bound, what)


def test_rejects_the_last_8_k_dropped():
    a, b, (ref, bound) = _plain()
    _rejected(R.emulate(a[..., :-8], b[..., :-8, :]), ref, bound, "last 8 k dropped")


def test_rejects_one_k_dropped():
    a, b, (ref, bound) = _plain()
    for k in (0, 131, 263):
        keep = [i for i in range(264) if i != k]
        _rejected(R.emulate(a[..., keep], b[..., keep, :]), ref, bound, f"k = {k} dropped")


def test_rejects_one_k_dropped_in_one_8_wide_remnant_only():
    """The defect confined to the 8-wide column remnant of a single batch entry: 8 x 200 elements out of 800 000."""
    a, b, (ref, bound) = _plain()
    out = R.emulate(a, b)
    out[1, 2, :, -8:] = R.emulate(a[1, 2, :, :-1], b[1, 2, :-1, -8:])
    _rejected(out, ref, bound, "one k dropped in one remnant")


def test_rejects_the_last_ragged_row_block_shifted_by_one_row():
    a, b, (ref, bound) = _plain()
    out = R.emulate(a, b)
    out[..., 192:, :] = out[..., 192:, :].roll(1, dims=-2)
    _rejected(out, ref, bound, "row block shifted")


def test_rejects_the_last_8_columns_of_the_neighbouring_batch_entry():
    a, b, (ref, bound) = _plain()
    out = R.emulate(a, b)
    flat = out.reshape(OUTER * INNER, 200, 136)
    flat[:, :, -8:] = flat.roll(1, dims=0)[:, :, -8:].clone()
    _rejected(out, ref, bound, "columns of the neighbour entry")


def test_rejects_swapped_batch_levels():
    """z1 and z2 exchanged on a square batch (only then does the swap stay in range)."""
    a, b = _rnd(3, 3, 200, 264, seed=1), _rnd(3, 3, 264, 136, seed=2, scale=0.05)
    ref, bound = R.reference(a, b)
    _rejected(R.emulate(a, b).transpose(0, 1), ref, bound, "z1 / z2 swapped")


def test_rejects_an_empty_split_k_slice_replaced_by_a_copy_of_slice_0():
    """(200, 136, 264) / 4 -> k_chunk 128: slices of 128, 128, 8 and an empty one; the empty one's workspace holding slice 0 again."""
    a, b, (ref, bound) = _plain()
    acc = R.accumulate(a, b, F32, k_chunk=128)
    R.assert_within(R.epilogue(acc), ref, bound, "split 4")
    stale = acc + a[..., :128].float() @ b[..., :128, :].float()
    _rejected(R.epilogue(stale), ref, bound, "empty slice = slice 0")


def test_rejects_a_residual_read_with_the_wrong_batch_stride():
    M, N, K = 200, 136, 264
    a, b, _ = _case(M, N, K, "plain")
    s2 = M * N + 64
    s1 = INNER * s2 + 128
    store = _rnd(OUTER * s1, seed=7)
    res = R.view(store, M, N, N, outer=OUTER, inner=INNER, s1=s1, s2=s2)
    ref, bound = R.reference(a, b, residual=res)
    R.assert_within(R.emulate(a, b, residual=res), ref, bound, "residual, own strides")
    wrong = R.view(store, M, N, N, outer=OUTER, inner=INNER, s1=INNER * s2, s2=s2)  # the outer stride of an unpadded buffer
    _rejected(R.emulate(a, b, residual=wrong), ref, bound, "residual with C's outer stride")


def test_assert_within_reports_the_worst_element_and_exempts_none():
    ref = torch.ones(2, 3, 4, 5, dtype=F64)
    bound = torch.full_like(ref, 1e-3)
    out = ref.clone()
    assert R.assert_within(out, ref, bound, "exact") == 0.0
    out[1, 2, 3, 4] += 2e-3  # ONE element of 120
    with pytest.raises(AssertionError, match=r"1 of 120 elements.*batch \(1, 2\) row 3 col 4"):
        R.assert_within(out, ref, bound, "one element")
    out[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="2 of 120"):
        R.assert_within(out, ref, bound, "nan")
