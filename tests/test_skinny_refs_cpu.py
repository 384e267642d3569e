"""tests/skinny_refs.py held against itself on the CPU: (a) the f32 emulation of every launch form of kai0_gemm_skinny_bf16 stays inside
the derived per-element bound at the shapes of tests/test_skinny_gpu.py, (b) the exact-input construction of the adaRMS prologue does
what its derivation says, and (c) the defects the GPU file exists to catch — a dropped K chunk in one column tile, exchanged pair
columns, a shifted ragged row tile, a neighbour entry's gate / modulation / rstd, a missing partial, wrong RoPE rows, a rotated or
shifted value segment — are rejected when planted into the emulation.  No HIP library, no GPU."""

import functools

import pytest
import torch

import skinny_refs as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
WORST = {}


def note(form, what, w):
    WORST[form] = max(WORST.get(form, 0.0), w)
    print(f"[{form}] {what}: worst err / bound {w:.3f} (form so far {WORST[form]:.3f})")


def _rejected(out, ref, bound, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        R.assert_within(out, ref, bound, what)


def _gate_rows(gate, rpb, M):
    return gate.repeat_interleave(rpb, 0)[:M]


# ------------------------------------------------------------------------------------------------ the emulation inside the bound
@pytest.mark.parametrize("K", R.MODE0_K)
def test_mode0_emulation_stays_within_the_bound(K):
    """Linear epilogue (gate + residual, residual only, neither), every M of the GPU file, and rowsq_out from the stored rows."""
    for M, amap in R.MODE0_MAPS:
        for N in R.MODE0_N:
            a, w = R.rnd(M, K, seed=1), R.rnd(N, K, seed=2, scale=0.05)
            rpb = amap[0] if amap else M
            gate, res = _gate_rows(R.rnd((M + rpb - 1) // rpb, N, seed=3), rpb, M), R.rnd(M, N, seed=4)
            acc64, acc32 = R.product(a, w, F64), R.product(a, w, F32)
            for name, kw in (("gate+residual", dict(gate=gate, residual=res)), ("residual", dict(residual=res)), ("plain", {})):
                out = R.linear(*acc32, **kw)
                note("mode 0", f"{name} {M}x{N}x{K}", R.assert_within(out, *R.linear(*acc64, **kw), f"{name} {M}x{N}x{K}"))
            sq = (out.float() * out.float()).reshape(M, N // 16, 16).sum(-1).t()  # f32, 16 addends in order
            note("rowsq_out", f"{M}x{N}x{K}", R.assert_within(sq, *R.rowsq_out_ref(out), "rowsq_out"))


@pytest.mark.parametrize("k_blk", R.K_BLK)
@pytest.mark.parametrize("split", [2, 4])
def test_split_k_partials_stay_within_their_slice_bound(k_blk, split):
    K, N = k_blk * split, 128
    for M in R.SPLIT_M:
        a, w = R.rnd(M, K, seed=1), R.rnd(N, K, seed=2, scale=0.05)
        ref, bound = R.partials(a, w, split, F64)
        note("split-K partials", f"{M}x{N}x{K}/{split}", R.assert_within(R.partials(a, w, split, F32)[0], ref, bound, "partials"))


@functools.lru_cache(maxsize=None)
def _qkv(H, HD, B, Hs, parts=3):
    """Logical inputs of a folded q|k|v case and its f64 / f32 accumulators."""
    K, M, N = 1024, B * Hs, (H + 2) * HD
    x, w = R.rnd(M, K, seed=1), R.rnd(N, K, seed=2, scale=0.05)
    cvec = R.rnd(N, seed=3, scale=0.5, dtype=F32)
    P, S_ld = 5, 5 + Hs + 6
    cos, sin = R.rope_tables(B * S_ld, HD // 2, seed=4)  # (the launch gets the first M rows: the tables are indexed by the A row)
    return dict(K=K, M=M, N=N, x=x, w=w, cvec=cvec, cos=cos, sin=sin, cmap=(Hs, S_ld, P), rowsq=R.rowsq_partials(x, parts, seed=5),
                acc64=R.product(x, w, F64), acc32=R.product(x, w, F32))


@pytest.mark.parametrize("H,HD", R.QKV_HEADS)
def test_folded_qkv_emulation_stays_within_the_bound(H, HD):
    for B, Hs in R.QKV_BATCH:
        for parts in R.QKV_PARTS:
            c = _qkv(H, HD, B, Hs, parts)
            M, segs = c["M"], R.qkv_segs(H, HD)
            refs = R.segments(*R.fold(*c["acc64"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
            outs = R.segments(*R.fold(*c["acc32"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
            for out, (ref, bound), name in zip(outs, refs, "qkv"):
                note("folded q|k|v " + ("rope" if name != "v" else "plain"), f"{name} H={H} HD={HD} B={B} Hs={Hs} parts={parts}",
                     R.assert_within(out, ref, bound, name))


@pytest.mark.parametrize("F,M", R.GEGLU_CASES)
def test_folded_geglu_emulation_stays_within_the_bound(F, M):
    K = 1024
    x, w = R.rnd(M, K, seed=1), R.rnd(2 * F, K, seed=2, scale=0.05)
    cvec = R.rnd(2 * F, seed=3, scale=0.5, dtype=F32)
    acc64, acc32 = R.product(x, w, F64), R.product(x, w, F32)
    for parts in R.GEGLU_PARTS:
        rowsq = R.rowsq_partials(x, parts, seed=5)
        out = R.geglu(*R.fold(*acc32, rowsq, cvec, K))
        note("folded GeGLU", f"F={F} M={M} parts={parts}", R.assert_within(out, *R.geglu(*R.fold(*acc64, rowsq, cvec, K)), "h"))
    note("plain GeGLU", f"F={F} M={M}", R.assert_within(R.geglu(*acc32), *R.geglu(*acc64), "h plain"))


@functools.lru_cache(maxsize=None)
def _ada(B, rpb, short, N, seed=7):
    K, M = 1024, B * rpb - short
    x, scale, shift = R.exact_ada_inputs(M, K, B, seed=seed)
    w = R.rnd(N, K, seed=2, scale=0.05)
    y, ey = R.ada_exact(x, scale, shift, rpb)
    return dict(K=K, M=M, x=x, scale=scale, shift=shift, w=w, y=y, ey=ey)


@pytest.mark.parametrize("B,rpb,short", R.ADA_CASES)
def test_adarms_prologue_emulation_stays_within_the_bound(B, rpb, short):
    H, HD, F = 2, 256, 272
    c = _ada(B, rpb, short, (H + 2) * HD)
    M = c["M"]
    cos, sin = R.rope_tables(M, HD // 2, seed=4)
    y32 = R.ada_emulate(c["x"], c["scale"], c["shift"], rpb)
    refs = R.segments(*R.product(c["y"], c["w"], F64, ey=c["ey"]), R.qkv_segs(H, HD), cos, sin)
    outs = R.segments(*R.product(y32, c["w"], F32), R.qkv_segs(H, HD), cos, sin)
    for out, (ref, bound), name in zip(outs, refs, "qkv"):
        note("adaRMS q|k|v", f"{name} B={B} rpb={rpb} M={M}", R.assert_within(out, ref, bound, name))
    g = _ada(B, rpb, short, 2 * F)
    out = R.geglu(*R.product(y32, g["w"], F32))
    note("adaRMS GeGLU", f"B={B} rpb={rpb} M={M}", R.assert_within(out, *R.geglu(*R.product(g["y"], g["w"], F64, ey=g["ey"])), "h"))


def test_plain_mode_1_and_2_emulation_stays_within_the_bound():
    """The unfolded modes 1 / 2 of the block-split kernels and of the plain in-block kernel, K = 512 and 1024."""
    H, HD, F = 3, 32, 48
    for K in R.K_BLK:
        for M in R.SPLIT_M:
            x = R.rnd(M, K, seed=1)
            cos, sin = R.rope_tables(M, HD // 2, seed=4)
            w = R.rnd((H + 2) * HD, K, seed=2, scale=0.05)
            for out, (ref, bound), name in zip(R.segments(*R.product(x, w, F32), R.qkv_segs(H, HD), cos, sin),
                                               R.segments(*R.product(x, w, F64), R.qkv_segs(H, HD), cos, sin), "qkv"):
                note("plain q|k|v", f"{name} M={M} K={K}", R.assert_within(out, ref, bound, name))
            w = R.rnd(2 * F, K, seed=3, scale=0.05)
            note("plain GeGLU", f"M={M} K={K}", R.assert_within(R.geglu(*R.product(x, w, F32)), *R.geglu(*R.product(x, w, F64)), "h"))


# ------------------------------------------------------------------------------------------------ the constants and the construction
def test_gelu_lipschitz_constant_covers_the_derivative():
    """sup |gelu_tanh'| recomputed in f64 on a grid of step 1e-4 over [-12, 12] (beyond it the derivative is 0 or 1 to 1e-30)."""
    x = torch.linspace(-12.0, 12.0, 240001, dtype=F64, requires_grad=True)
    torch.nn.functional.gelu(x, approximate="tanh").sum().backward()
    sup = float(x.grad.abs().max())
    print(f"sup |gelu_tanh'| = {sup:.6f} at x = {float(x.detach()[x.grad.abs().argmax()]):.4f}")
    assert 1.128 < sup <= R.L_GELU


def test_fast_gelu_of_the_emulation_is_within_its_allowance():
    """common.h's form in f32 against the f64 gelu: inside |g| (SIG_ERR + 8 U32), the allowance the GeGLU bound grants it."""
    g = R.S.gelu_points(4096).float()
    g = g[g.abs() <= 100.0]
    ref = torch.nn.functional.gelu(g.to(F64), approximate="tanh")
    err = (R.gelu_fast(g).to(F64) - ref).abs()
    allow = g.to(F64).abs() * (R.SIG_ERR + 8 * R.U32) + R.TINY
    print(f"fast gelu: worst err / allowance {float((err / allow).max()):.3f}")
    assert bool((err <= allow).all())


def test_exact_adarms_inputs_make_the_prologue_exact():
    """M = 130, K = 1024, two entries of 65 rows: the mean square of every row is exactly 4^j, every exact y is a bf16 value, the f32
    prologue reproduces it bit for bit where y != 0 and stays within e_y where y = 0; the f64 adaRMS with eps agrees with the exact y
    to eps / (2 meansq)."""
    M, K, B, rpb = 130, 1024, 2, 65
    x, scale, shift = R.exact_ada_inputs(M, K, B, seed=7)
    ms = x.double().pow(2).mean(-1)
    assert bool((torch.log2(ms) / 2 == torch.round(torch.log2(ms) / 2)).all()) and set(torch.log2(ms).div(2).int().tolist()) == {-2, -1, 0, 1, 2}
    y, ey = R.ada_exact(x, scale, shift, rpb)
    assert bool((y.to(BF16).double() == y).all()) and float(y.abs().max()) <= 5.0 and bool((y * 16 == torch.round(y * 16)).all())
    y32 = R.ada_emulate(x, scale, shift, rpb).double()
    nz = y != 0
    assert bool((y32[nz] == y[nz]).all()), f"{int((y32[nz] != y[nz]).sum())} non-zero elements not reproduced"
    assert bool(((y32 - y).abs()[~nz] <= ey[~nz]).all()) and bool((ey[nz] == 0).all())
    print(f"exact y: {int((~nz).sum())} zeros of {y.numel()}, worst |y32| there {float(y32[~nz].abs().max()):.3g} "
          f"(worst / e_y {float((y32[~nz].abs() / ey[~nz]).max()):.3f})")
    y_eps = R.rmsnorm_fwd(x, None, R.EPS, F64, mod=torch.cat([scale, shift], 1), rpb=rpb)["y"].value
    lim = R.EPS / (2 * ms[:, None]) * 1.001 * (y.abs() + shift.double().repeat_interleave(rpb, 0).abs()) + 1e-15
    assert bool(((y_eps - y).abs() <= lim).all())


def test_pack_index_is_a_permutation_of_1_kib_blocks():
    idx = R.pack_index(48, 96)
    assert sorted(idx.reshape(-1).tolist()) == list(range(48 * 96))
    assert int(idx[16 * 2 + 5, 32 * 1 + 8 * 3 + 6]) == (2 * 3 + 1) * 512 + (5 + 16 * 3) * 8 + 6


# ------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("K", R.MODE0_K)
def test_rejects_one_128_wide_k_chunk_dropped_in_one_column_tile(K):
    """1. mode 0 at M = 50, N = 384: a wave's chunk [K - 256, K - 128) missing from the 16 columns of tile 5 only."""
    a, w = R.rnd(50, K, seed=1), R.rnd(384, K, seed=2, scale=0.05)
    ref, bound = R.linear(*R.product(a, w, F64))
    acc, _ = R.product(a, w, F32)
    R.assert_within(R.linear(acc, None), ref, bound, "intact")
    ks = slice(K - 256, K - 128)
    acc[:, 80:96] -= a[:, ks].float() @ w[80:96, ks].float().t()
    _rejected(R.linear(acc, None), ref, bound, "chunk dropped in tile 5")


def _swap(acc, n, stride, width=16):
    out = acc.clone()
    out[:, n : n + width], out[:, n + stride : n + stride + width] = acc[:, n + stride : n + stride + width], acc[:, n : n + width]
    return out


def test_rejects_pair_columns_exchanged_in_one_tile():
    """2. columns n and n + pair_stride of one 16-column tile exchanged: the RoPE partner (folded q|k|v), the GeGLU gate / up pair,
    and the two 16-column groups of a block-split mode-0 block."""
    H, HD = 2, 256
    c = _qkv(H, HD, 1, 50)
    M, segs = c["M"], R.qkv_segs(H, HD)
    refs = R.segments(*R.fold(*c["acc64"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
    bad = R.segments(*R.fold(_swap(c["acc32"][0], HD + 32, HD // 2), None, c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
    _rejected(bad[0], *refs[0], "RoPE partner exchanged")
    R.assert_within(bad[1], *refs[1], "k is intact")
    F = 272
    x, w = R.rnd(65, 1024, seed=1), R.rnd(2 * F, 1024, seed=2, scale=0.05)
    _rejected(R.geglu(_swap(R.product(x, w, F32)[0], 256, F), None), *R.geglu(*R.product(x, w, F64)), "gate / up exchanged")
    w = R.rnd(128, 1024, seed=2, scale=0.05)
    _rejected(R.linear(_swap(R.product(x, w, F32)[0], 32, 16), None), *R.linear(*R.product(x, w, F64)), "mode 0 groups exchanged")


def test_rejects_the_ragged_last_row_tile_shifted_by_one_row():
    """3. M = 130: the last 16-row tile holds rows 128, 129."""
    a, w = R.rnd(130, 1024, seed=1), R.rnd(128, 1024, seed=2, scale=0.05)
    out = R.linear(*R.product(a, w, F32))
    out[128:] = out[128:].roll(1, dims=0)
    _rejected(out, *R.linear(*R.product(a, w, F64)), "last row tile shifted")


def test_rejects_the_first_row_of_entry_1_gated_with_entry_0():
    """4. M = 102, rpb = 51: row 51 multiplied by gate[0]."""
    M, N, rpb = 102, 128, 51
    a, w = R.rnd(M, 1024, seed=1), R.rnd(N, 1024, seed=2, scale=0.05)
    gate, res = _gate_rows(R.rnd(2, N, seed=3), rpb, M), R.rnd(M, N, seed=4)
    ref, bound = R.linear(*R.product(a, w, F64), gate=gate, residual=res)
    wrong = gate.clone()
    wrong[rpb] = gate[0]
    R.assert_within(R.linear(*R.product(a, w, F32), gate=gate, residual=res), ref, bound, "intact")
    _rejected(R.linear(*R.product(a, w, F32), gate=wrong, residual=res), ref, bound, "row rpb with entry 0's gate")


def test_rejects_an_adarms_row_tile_normalised_with_the_neighbouring_entry():
    """5. (B, rpb) = (2, 17): the second row tile of entry 0 (its row 16 alone) takes entry 1's scale | shift."""
    B, rpb, F = 2, 17, 272
    c = _ada(B, rpb, 0, 2 * F)
    ref, bound = R.geglu(*R.product(c["y"], c["w"], F64, ey=c["ey"]))
    y32 = R.ada_emulate(c["x"], c["scale"], c["shift"], rpb)
    R.assert_within(R.geglu(*R.product(y32, c["w"], F32)), ref, bound, "intact")
    y32[16] = R.ada_emulate(c["x"][16:17], c["scale"][1:], c["shift"][1:], 1)[0]
    _rejected(R.geglu(*R.product(y32, c["w"], F32)), ref, bound, "row tile with the neighbour's modulation")


@pytest.mark.parametrize("parts", [3, 64])
def test_rejects_the_last_partial_not_added(parts):
    """6."""
    H, HD = 2, 256
    c = _qkv(H, HD, 1, 50, parts)
    M, segs = c["M"], R.qkv_segs(H, HD)
    refs = R.segments(*R.fold(*c["acc64"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
    bad = R.segments(*R.fold(*c["acc32"], c["rowsq"][:-1], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
    _rejected(bad[0], *refs[0], f"partial {parts - 1} of {parts} missing")
    _rejected(bad[2], *refs[2], f"partial {parts - 1} of {parts} missing (v)")


def test_rejects_rstd_of_the_next_row():
    """7. folded GeGLU: row 49 scaled with row 50's statistic (rows with different norms: x is scaled per row)."""
    F, M, K = 272, 65, 1024
    x = (R.rnd(M, K, seed=1).float() * (1.0 + 0.05 * torch.arange(M)[:, None])).to(BF16)
    w, cvec = R.rnd(2 * F, K, seed=2, scale=0.05), R.rnd(2 * F, seed=3, scale=0.5, dtype=F32)
    rowsq = R.rowsq_partials(x, 3, seed=5)
    ref, bound = R.geglu(*R.fold(*R.product(x, w, F64), rowsq, cvec, K))
    R.assert_within(R.geglu(*R.fold(*R.product(x, w, F32), rowsq, cvec, K)), ref, bound, "intact")
    wrong = rowsq.clone()
    wrong[:, 49] = rowsq[:, 50]
    _rejected(R.geglu(*R.fold(*R.product(x, w, F32), wrong, cvec, K)), ref, bound, "rstd of row r + 1")


def test_rejects_rope_tables_indexed_by_the_output_row():
    """8. the tables belong to the A row; the mapped output row (c_map) picks another position."""
    H, HD = 3, 32
    c = _qkv(H, HD, 2, 51)
    M, segs = c["M"], R.qkv_segs(H, HD)
    refs = R.segments(*R.fold(*c["acc64"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
    orow = R.row_index(M, c["cmap"])
    bad = R.segments(*R.fold(*c["acc32"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][orow], c["sin"][orow])
    _rejected(bad[0], *refs[0], "q rotated by the output row's position")
    _rejected(bad[1], *refs[1], "k rotated by the output row's position")
    R.assert_within(bad[2], *refs[2], "v is intact")


def test_rejects_a_rotated_value_segment():
    """9."""
    H, HD = 3, 32
    c = _qkv(H, HD, 1, 17)
    M = c["M"]
    refs = R.segments(*R.fold(*c["acc64"], c["rowsq"], c["cvec"], c["K"]), R.qkv_segs(H, HD), c["cos"][:M], c["sin"][:M])
    segs = [(nb, ne, 1) for nb, ne, _ in R.qkv_segs(H, HD)]
    bad = R.segments(*R.fold(*c["acc32"], c["rowsq"], c["cvec"], c["K"]), segs, c["cos"][:M], c["sin"][:M])
    _rejected(bad[2], *refs[2], "v rotated")


def test_rejects_the_transposed_value_store_one_row_off():
    """10. vt[b][col][P + t] written at P + t + 1: the window [P, P + Hs) then holds the neighbouring rows."""
    H, HD, B, Hs = 2, 256, 2, 51
    c = _qkv(H, HD, B, Hs)
    M, (_, S_ld, P) = c["M"], c["cmap"]
    v = R.segments(*R.fold(*c["acc32"], c["rowsq"], c["cvec"], c["K"]), R.qkv_segs(H, HD, 2), c["cos"][:M], c["sin"][:M])[2]
    ref, bound = R.segments(*R.fold(*c["acc64"], c["rowsq"], c["cvec"], c["K"]), R.qkv_segs(H, HD, 2), c["cos"][:M], c["sin"][:M])[2]
    vt = torch.full((B, HD, S_ld + 3), R.SENTINEL, dtype=BF16)
    vt[:, :, P : P + Hs] = v.view(B, Hs, HD).transpose(1, 2)
    R.assert_within(vt[:, :, P : P + Hs].transpose(1, 2).reshape(M, HD), ref, bound, "intact")
    vt[:, :, P + 1 : P + Hs + 1] = v.view(B, Hs, HD).transpose(1, 2)
    _rejected(vt[:, :, P : P + Hs].transpose(1, 2).reshape(M, HD), ref, bound, "vt one row off")
