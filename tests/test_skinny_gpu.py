"""kai0_gemm_skinny_bf16 — every projection of the denoise loop — held to the per-element float64 bound of tests/skinny_refs.py in each
of its launch forms: the in-block mode 0 of o_proj / down_proj (row-mapped A, packed weights, strided gate, row statistics), the
folded q|k|v + RoPE and gate|up + GeGLU launches of production, their adaRMS-prologue alternatives, the plain in-block modes 1 / 2
and the block-split kernels with their split-K partials; then every descriptor the entry point refuses.

Which of the ten instantiations a case reaches follows from (split_k, mode, K, mod, rowsq_in) — csrc/skinny.hip, skinny_inblock — and is
named in each test.  Every case launches into sentinel-filled storage with padded leading dimensions; everything outside the written
windows must come back unchanged, and every operand's padding holds NaN (skinny_refs: a launch that reads what it must not read
returns a non-finite value).  Inputs: A ~ N(0, 1), W ~ 0.05 N(0, 1), gate and residual ~ N(0, 1), seeded."""

import functools

import pytest
import torch

import skinny_refs as R

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
WORST = {}  # family -> worst err / bound seen (printed per test; profiles/HISTORY.md records a run)
PAD = 8


@pytest.fixture(scope="module")
def ops():
    from kai0_amd import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _rnd_cpu(shape, seed, scale, dtype):
    return R.rnd(*shape, seed=seed, scale=scale, dtype=dtype)


def rnd(*shape, seed, scale=1.0, dtype=BF16):
    return _rnd_cpu(shape, seed, scale, dtype).to(dev())


def note(family, what, w):
    WORST[family] = max(WORST.get(family, 0.0), w)
    print(f"[{family}] {what}: worst err / bound {w:.3f} (family so far {WORST[family]:.3f})")


def sentinel(*shape, dtype=BF16):
    return torch.full(shape, R.SENTINEL, dtype=dtype, device=dev())


def gate_rows(gate, rpb, M):
    return gate.repeat_interleave(rpb, 0)[:M]


# ------------------------------------------------------------------------------------------------ a. in-block mode 0
@pytest.mark.parametrize("K", R.MODE0_K)
@pytest.mark.parametrize("M,amap", R.MODE0_MAPS)
def test_inblock_mode0(ops, M, amap, K):
    """split_k = -1, mode 0: skinny2_kernel<K / 256, 1, false, false, 2, false, true> (o_proj, down_proj).  A read through the row map
    out of NaN-padded storage, with (strided gate + residual + rowsq_out), (residual only: the pi0 form) and neither; row-major
    and packed W give the same bits."""
    rpb = amap[0] if amap else M
    nb = (M + rpb - 1) // rpb
    a = rnd(M, K, seed=1)
    A = R.padded(a, amap)
    for N in R.MODE0_N:
        w, gate, res = rnd(N, K, seed=2, scale=0.05), rnd(nb, N, seed=3), rnd(M, N, seed=4)
        Ws = {False: R.padded(w), True: ops.pack_skinny_weight(w)}
        gview, gate_ld = R.strided(gate, 2 * N)
        Rs = R.padded(res)
        acc = R.product(a, w, F64)
        for form in ("gate+residual", "residual", "plain"):
            kw, ref_kw = {}, {}
            if form == "gate+residual":
                kw.update(gate=gview, gate_rpb=rpb, gate_ld=gate_ld)
                ref_kw.update(gate=gate_rows(gate, rpb, M))
            if form != "plain":
                kw.update(residual=Rs, ldr=N + PAD)
                ref_kw.update(residual=res)
            ref, bound = R.linear(*acc, **ref_kw)
            outs = []
            for packed in (False, True):
                out = sentinel(M, N + PAD)
                sq = sentinel(N // 16, M + 3, dtype=F32) if form == "gate+residual" else None
                ops.skinny_gemm(A, Ws[packed], M=M, N=N, K=K, lda=K + PAD, ldw=K + PAD, split_k=-1, segs=[(out, N + PAD, 0, N, 0)],
                                a_map=amap, w_packed=packed, rowsq_out=sq, **kw)
                torch.cuda.synchronize()
                what = f"{form} {M}x{N}x{K} a_map={amap} packed={packed}"
                note("a", what, R.assert_within(out[:, :N], ref, bound, what))
                R.assert_untouched(out, what, rows=slice(None), width=N)
                if sq is not None:
                    note("a rowsq_out", what, R.assert_within(sq[:, :M], *R.rowsq_out_ref(out[:, :N]), "rowsq_out " + what))
                    R.assert_untouched(sq, "rowsq_out " + what, rows=slice(None), width=M)
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), f"{form} {M}x{N}x{K}: row-major and packed W differ"


def test_pack_skinny_weight_is_the_headers_formula(ops):
    """ops.pack_skinny_weight against kai0hip.h's w_packed offsets, index by index and bit for bit."""
    for N, K in ((128, 1024), (48, 96), (384, 4096)):
        w = rnd(N, K, seed=2, scale=0.05)
        want = torch.empty(N * K, dtype=BF16, device=dev())
        want[R.pack_index(N, K).reshape(-1).to(dev())] = w.reshape(-1)
        assert torch.equal(ops.pack_skinny_weight(w).reshape(-1), want), (N, K)


# ------------------------------------------------------------------------------------------------ b. folded q|k|v + RoPE
class Qkv:
    """Destinations of a mode-1 q|k|v launch: q and k rows through c_map = (Hs, S_ld, P) into [B * S_ld][width + 8] buffers, v likewise
    (rope 0) or transposed into vt [B][HD][S_ld + 3] (rope 2)."""

    def __init__(self, H, HD, B, Hs, M=None, P=5):
        self.H, self.HD, self.B, self.Hs, self.P = H, HD, B, Hs, P
        self.M = B * Hs if M is None else M
        self.N, self.S_ld, self.vt_ld = (H + 2) * HD, P + Hs + 6, P + Hs + 6 + 3
        self.cmap = (Hs, self.S_ld, P)
        self.rows = R.row_index(self.M, self.cmap, dev())

    def launch(self, ops, A, W, v_rope, cos, sin, **kw):
        H, HD, S = self.H, self.HD, self.B * self.S_ld
        self.q, self.k = sentinel(S, H * HD + PAD), sentinel(S, HD + PAD)
        self.v = sentinel(self.B, HD, self.vt_ld) if v_rope == 2 else sentinel(S, HD + PAD)
        lds = (H * HD + PAD, HD + PAD, self.vt_ld if v_rope == 2 else HD + PAD)
        segs = [(d, ld, nb, ne, rp) for d, ld, (nb, ne, rp) in zip((self.q, self.k, self.v), lds, R.qkv_segs(H, HD, v_rope))]
        ops.skinny_gemm(A, W, M=self.M, N=self.N, mode=1, pair_stride=HD // 2, segs=segs, c_map=self.cmap, rope_cos=cos,
                        rope_sin=sin, rope_half=HD // 2, **kw)
        torch.cuda.synchronize()

    def check(self, refs, v_rope, family, what):
        H, HD, M = self.H, self.HD, self.M
        for name, store, width, (ref, bound) in (("q", self.q, H * HD, refs[0]), ("k", self.k, HD, refs[1])):
            note(family, f"{name} {what}", R.assert_within(store[self.rows, :width], ref, bound, f"{name} {what}"))
            R.assert_untouched(store, f"{name} {what}", rows=self.rows, width=width)
        ref, bound = refs[2]
        if v_rope != 2:
            note(family, f"v {what}", R.assert_within(self.v[self.rows, :HD], ref, bound, f"v {what}"))
            R.assert_untouched(self.v, f"v {what}", rows=self.rows, width=HD)
            return
        # vt[b][col][P + t] = v[b * Hs + t][col]; the last entry may be short
        region = torch.zeros(self.B, HD, self.vt_ld, dtype=torch.bool, device=dev())
        got = torch.empty(M, HD, dtype=BF16, device=dev())
        for b in range(self.B):
            n = min(self.Hs, M - b * self.Hs)
            region[b, :, self.P : self.P + n] = True
            got[b * self.Hs : b * self.Hs + n] = self.v[b, :, self.P : self.P + n].t()
        note(family, f"vt {what}", R.assert_within(got, ref, bound, f"vt {what}"))
        R.assert_untouched(self.v, f"vt {what}", region=region)


@pytest.mark.parametrize("B,Hs", R.QKV_BATCH)
@pytest.mark.parametrize("H,HD", R.QKV_HEADS)
def test_folded_qkv_rope(ops, H, HD, B, Hs):
    """split_k = -1, mode 1, rowsq_in: skinny2_kernel<8, 1, true, false, 1, false, true, true>, the production q|k|v launch.  Three
    column segments (q and k rotated, v plain or stored transposed) through c_map; rstd from 1, 3 and 64 partials out of a
    [parts][M + 3] buffer whose last columns hold NaN; row-major and packed W give the same bits."""
    K = 1024
    d = Qkv(H, HD, B, Hs)
    M, N = d.M, d.N
    x, w, cvec = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05), rnd(N, seed=3, scale=0.5, dtype=F32)
    cos, sin = (t.to(dev()) for t in R.rope_tables(M, HD // 2, seed=4))
    A, Ws = R.padded(x), {False: R.padded(w), True: ops.pack_skinny_weight(w)}
    acc = R.product(x, w, F64)
    for parts in R.QKV_PARTS:
        rowsq = R.rowsq_partials(x, parts, seed=5)
        folded = R.fold(*acc, rowsq, cvec, K)
        for v_rope in (0, 2):
            refs = R.segments(*folded, R.qkv_segs(H, HD, v_rope), cos, sin)
            outs = []
            for packed in (False, True):
                d.launch(ops, A, Ws[packed], v_rope, cos, sin, K=K, lda=K + PAD, ldw=K + PAD, split_k=-1, w_packed=packed,
                         rowsq_in=R.padded(rowsq, pad=3), rowsq_parts=parts, cvec=cvec, eps=R.EPS)
                d.check(refs, v_rope, "b", f"H={H} HD={HD} B={B} Hs={Hs} parts={parts} v_rope={v_rope} packed={packed}")
                outs.append((d.q, d.k, d.v))
            assert all(torch.equal(s, t) for s, t in zip(*outs)), "row-major and packed W differ"


# ------------------------------------------------------------------------------------------------ c. folded gate|up + GeGLU
@pytest.mark.parametrize("F,M", R.GEGLU_CASES)
def test_folded_geglu(ops, F, M):
    """split_k = -1, mode 2, rowsq_in: skinny2_kernel<8, 4, true, false, 1, true, true, true>, the production gate|up launch."""
    K = 1024
    x, w, cvec = rnd(M, K, seed=1), rnd(2 * F, K, seed=2, scale=0.05), rnd(2 * F, seed=3, scale=0.5, dtype=F32)
    A, Ws = R.padded(x), {False: R.padded(w), True: ops.pack_skinny_weight(w)}
    acc = R.product(x, w, F64)
    for parts in R.GEGLU_PARTS:
        rowsq = R.rowsq_partials(x, parts, seed=5)
        ref, bound = R.geglu(*R.fold(*acc, rowsq, cvec, K))
        outs = []
        for packed in (False, True):
            h = sentinel(M, F + PAD)
            ops.skinny_gemm(A, Ws[packed], M=M, N=2 * F, K=K, lda=K + PAD, ldw=K + PAD, mode=2, pair_stride=F, split_k=-1,
                            segs=[(h, F + PAD, 0, F, 0)], w_packed=packed, rowsq_in=R.padded(rowsq, pad=3), rowsq_parts=parts, cvec=cvec,
                            eps=R.EPS)
            torch.cuda.synchronize()
            what = f"F={F} M={M} parts={parts} packed={packed}"
            note("c", what, R.assert_within(h[:, :F], ref, bound, what))
            R.assert_untouched(h, what, rows=slice(None), width=F)
            outs.append(h)
        assert torch.equal(outs[0], outs[1]), "row-major and packed W differ"


# ------------------------------------------------------------------------------------------------ d. adaRMS prologue
@pytest.mark.parametrize("B,rpb,short", R.ADA_CASES)
def test_adarms_prologue(ops, B, rpb, short):
    """split_k = -1 with `mod`: skinny2_kernel<8, 1, true, true, 1, false, true> (mode 1) and <8, 4, true, true, 1, true, true> (mode 2),
    the A/B alternatives of the folded launches, on the inputs that make the prologue exact (skinny_refs).  Row tiles start at every
    entry (m0 = b * rpb + t * TMB); `mod` is a strided view with mod_ld = 4 K + 8 > 3 K between NaN neighbours; short = 3: the last
    entry lacks three rows, and at rpb = 17 its second row tile is empty."""
    K, H, HD, F = 1024, 2, 256, 272
    M = B * rpb - short
    x, scale, shift = R.exact_ada_inputs(M, K, B, seed=7, device=dev())
    y, ey = R.ada_exact(x, scale, shift, rpb)
    mod, mod_ld = R.strided(torch.cat([scale, shift], 1), K, after=K + 8)
    A = R.padded(x)
    ada = dict(K=K, lda=K + PAD, ldw=K + PAD, split_k=-1, mod=mod, mod_ld=mod_ld, mod_rpb=rpb, eps=R.EPS)
    # mode 1
    d = Qkv(H, HD, B, rpb, M=M)
    w = rnd(d.N, K, seed=2, scale=0.05)
    cos, sin = (t.to(dev()) for t in R.rope_tables(M, HD // 2, seed=4))
    refs = R.segments(*R.product(y, w, F64, ey=ey), R.qkv_segs(H, HD, 2), cos, sin)
    outs = []
    for packed, W in ((False, R.padded(w)), (True, ops.pack_skinny_weight(w))):
        d.launch(ops, A, W, 2, cos, sin, w_packed=packed, **ada)
        d.check(refs, 2, "d", f"mode 1 B={B} rpb={rpb} M={M} packed={packed}")
        outs.append((d.q, d.k, d.v))
    assert all(torch.equal(s, t) for s, t in zip(*outs)), "row-major and packed W differ"
    # mode 2
    w = rnd(2 * F, K, seed=3, scale=0.05)
    ref, bound = R.geglu(*R.product(y, w, F64, ey=ey))
    outs = []
    for packed, W in ((False, R.padded(w)), (True, ops.pack_skinny_weight(w))):
        h = sentinel(M, F + PAD)
        ops.skinny_gemm(A, W, M=M, N=2 * F, mode=2, pair_stride=F, segs=[(h, F + PAD, 0, F, 0)], w_packed=packed, **ada)
        torch.cuda.synchronize()
        what = f"mode 2 B={B} rpb={rpb} M={M} packed={packed}"
        note("d", what, R.assert_within(h[:, :F], ref, bound, what))
        R.assert_untouched(h, what, rows=slice(None), width=F)
        outs.append(h)
    assert torch.equal(outs[0], outs[1]), "row-major and packed W differ"


# ------------------------------------------------------------------------------------------------ e. plain in-block 1 / 2, block-split
E_RPB, E_SLD, E_OFF = 43, 52, 4  # row map of family e: entries of 43 rows in 52-row slots from row 4


@pytest.mark.parametrize("M", R.SPLIT_M)
@pytest.mark.parametrize("k_blk", R.K_BLK)
def test_block_split_mode0(ops, k_blk, M):
    """split_k = 1, K = k_blk: skinny_kernel<1, 4> (512) / <2, 4> (1024), 64-row tiles.  pair_stride 16 and 64, A through a_map, gate
    and residual with the output through c_map (the residual's rows outside the windows hold NaN)."""
    K = k_blk
    rmap = (E_RPB, E_SLD, E_OFF)
    nb = (M + E_RPB - 1) // E_RPB
    a = rnd(M, K, seed=1)
    A = R.padded(a, rmap)
    rows = R.row_index(M, rmap, dev())
    for ps, N in ((16, 96), (64, 256)):
        w, gate, res = rnd(N, K, seed=2, scale=0.05), rnd(nb, N, seed=3), rnd(M, N, seed=4)
        gview, gate_ld = R.strided(gate, 2 * N)
        ref, bound = R.linear(*R.product(a, w, F64), gate=gate_rows(gate, E_RPB, M), residual=res)
        out = sentinel(nb * E_SLD, N + PAD)
        ops.skinny_gemm(A, R.padded(w), M=M, N=N, K=K, lda=K + PAD, ldw=K + PAD, pair_stride=ps, segs=[(out, N + PAD, 0, N, 0)],
                        a_map=rmap, c_map=rmap, gate=gview, gate_rpb=E_RPB, gate_ld=gate_ld, residual=R.padded(res, rmap), ldr=N + PAD)
        torch.cuda.synchronize()
        what = f"block-split mode 0 {M}x{N}x{K} pair_stride={ps}"
        note("e", what, R.assert_within(out[rows, :N], ref, bound, what))
        R.assert_untouched(out, what, rows=rows, width=N)


@pytest.mark.parametrize("M", R.SPLIT_M)
@pytest.mark.parametrize("split", [2, 4])
@pytest.mark.parametrize("k_blk", R.K_BLK)
def test_split_k_partials(ops, k_blk, split, M):
    """split_k = 2 / 4, K = split * k_blk: skinny_kernel<1, 4> / <2, 4> writing raw f32 partials [split][M][N].  Each slice against
    its own bound; 64 sentinel floats before and after the workspace stay."""
    K, N, band = split * k_blk, 128, 64
    rmap = (E_RPB, E_SLD, E_OFF)
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.05)
    ref, bound = R.partials(a, w, split, F64)
    buf = sentinel(band + split * M * N + band, dtype=F32)
    ws = buf[band : band + split * M * N]
    ops.skinny_gemm(R.padded(a, rmap), R.padded(w), M=M, N=N, K=K, lda=K + PAD, ldw=K + PAD, pair_stride=16, split_k=split, workspace=ws,
                    a_map=rmap)
    torch.cuda.synchronize()
    what = f"partials {M}x{N}x{K}/{split}"
    note("e split-K", what, R.assert_within(ws.view(split, M, N), ref, bound, what))
    assert bool((buf[:band] == R.SENTINEL).all()) and bool((buf[-band:] == R.SENTINEL).all()), f"{what}: a write outside the workspace"


@pytest.mark.parametrize("M", R.SPLIT_M)
def test_plain_inblock_mode_1_and_2(ops, M):
    """split_k = -1, K = 1024, no `mod`, no rowsq_in: skinny2_kernel<4, 4, true, false> (A fragments straight from global)."""
    K, H, HD, F = 1024, 3, 32, 48
    _mode_1_and_2(ops, M, K, H, HD, F, -1, "in-block plain")


@pytest.mark.parametrize("k_blk", R.K_BLK)
def test_block_split_mode_1_and_2(ops, k_blk):
    """split_k = 1, modes 1 and 2 once per k_blk at M = 65 (two 64-row tiles): skinny_kernel<1, 4> / <2, 4>."""
    _mode_1_and_2(ops, 65, k_blk, 3, 32, 48, 1, "block-split")


def _mode_1_and_2(ops, M, K, H, HD, F, split_k, name):
    B = 2 if M > 1 else 1
    Hs = (M + B - 1) // B
    x = rnd(M, K, seed=1)
    A = R.padded(x)
    d = Qkv(H, HD, B, Hs, M=M)
    w = rnd(d.N, K, seed=2, scale=0.05)
    cos, sin = (t.to(dev()) for t in R.rope_tables(M, HD // 2, seed=4))
    acc = R.product(x, w, F64)
    for v_rope in (0, 2):
        d.launch(ops, A, R.padded(w), v_rope, cos, sin, K=K, lda=K + PAD, ldw=K + PAD, split_k=split_k)
        d.check(R.segments(*acc, R.qkv_segs(H, HD, v_rope), cos, sin), v_rope, "e", f"{name} mode 1 M={M} K={K} v_rope={v_rope}")
    w = rnd(2 * F, K, seed=3, scale=0.05)
    h = sentinel(M, F + PAD)
    ops.skinny_gemm(A, R.padded(w), M=M, N=2 * F, K=K, lda=K + PAD, ldw=K + PAD, mode=2, pair_stride=F, split_k=split_k,
                    segs=[(h, F + PAD, 0, F, 0)])
    torch.cuda.synchronize()
    what = f"{name} mode 2 M={M} K={K}"
    note("e", what, R.assert_within(h[:, :F], *R.geglu(*R.product(x, w, F64)), what))
    R.assert_untouched(h, what, rows=slice(None), width=F)


# ------------------------------------------------------------------------------------------------ f. rejected descriptors
class Pool:
    """Operands large enough for every shape named below, so a descriptor that were accepted by mistake would still stay in bounds."""

    def __init__(self):
        self.A, self.W = rnd(136, 4104, seed=1), rnd(1160, 4104, seed=2, scale=0.05)
        self.out = sentinel(136, 1168)
        self.gate, self.res = rnd(4, 1168, seed=3), rnd(136, 1168, seed=4)
        self.cos, self.sin = (t.to(dev()) for t in R.rope_tables(136, 16, seed=4))
        self.mod = rnd(4, 3 * 4104, seed=5, scale=0.3, dtype=F32)
        self.rowsq = torch.ones(64, 64, dtype=F32, device=dev())
        self.cvec = rnd(1168, seed=6, dtype=F32)
        self.sq_out = sentinel(80, 64, dtype=F32)
        self.ws = sentinel(4 * 64 * 1168 + 8, dtype=F32)


M0 = 50


def _forms(p):
    """Valid descriptors of each launch form (M = 50), the starting points of the refused ones."""
    o = p.out
    qkv = [(o, 1168, 0, 96, 1), (o, 1168, 96, 128, 1), (o, 1168, 128, 160, 0)]
    rope = dict(rope_cos=p.cos, rope_sin=p.sin, rope_half=16)
    fold = dict(rowsq_in=p.rowsq, rowsq_parts=3, cvec=p.cvec, eps=R.EPS)
    ada = dict(mod=p.mod, mod_ld=3 * 4104, mod_rpb=25, eps=R.EPS)
    return {
        "block0": dict(M=M0, N=64, K=512, lda=4104, ldw=4104, pair_stride=16, segs=[(o, 1168, 0, 64, 0)]),
        "block1": dict(M=M0, N=160, K=512, lda=4104, ldw=4104, mode=1, pair_stride=16, segs=qkv, **rope),
        "block2": dict(M=M0, N=96, K=512, lda=4104, ldw=4104, mode=2, pair_stride=48, segs=[(o, 1168, 0, 48, 0)]),
        "splitk": dict(M=M0, N=64, K=1024, lda=4104, ldw=4104, pair_stride=16, split_k=2, workspace=p.ws[: 2 * M0 * 64]),
        "in0": dict(M=M0, N=128, K=1024, lda=4104, ldw=4104, split_k=-1, segs=[(o, 1168, 0, 128, 0)]),
        "in2": dict(M=M0, N=96, K=1024, lda=4104, ldw=4104, mode=2, pair_stride=48, split_k=-1, segs=[(o, 1168, 0, 48, 0)]),
        "fold1": dict(M=M0, N=160, K=1024, lda=4104, ldw=4104, mode=1, pair_stride=16, split_k=-1, segs=qkv, **rope, **fold),
        "fold2": dict(M=M0, N=96, K=1024, lda=4104, ldw=4104, mode=2, pair_stride=48, split_k=-1, segs=[(o, 1168, 0, 48, 0)], **fold),
        "ada2": dict(M=M0, N=96, K=1024, lda=4104, ldw=4104, mode=2, pair_stride=48, split_k=-1, segs=[(o, 1168, 0, 48, 0)], **ada),
    }


def _seg(p, *cols_rope, ld=1168):
    return [(p.out, ld, nb, ne, rp) for nb, ne, rp in cols_rope]


# (name, form, what to change (a function of the pool), the message of the KAI0_REQUIRE it must hit)
REFUSED = [
    ("M = 0", "block0", lambda p: dict(M=0), "unsupported"),
    ("N = 16", "block0", lambda p: dict(N=16), "unsupported"),
    ("N % 32", "block0", lambda p: dict(N=48), "unsupported"),
    ("K / split_k = 768", "block0", lambda p: dict(K=768), "must be 512 or 1024"),
    ("K / split_k = 2048", "block0", lambda p: dict(K=2048), "must be 512 or 1024"),
    ("K % split_k", "splitk", lambda p: dict(split_k=3, workspace=p.ws), "must be 512 or 1024"),
    ("lda % 8", "block0", lambda p: dict(lda=4100), "16-byte aligned"),
    ("ldw % 8", "block0", lambda p: dict(ldw=4108), "16-byte aligned"),
    ("A misaligned", "block0", lambda p: dict(A=p.A.view(-1)[1:]), "16-byte aligned"),
    ("W misaligned", "block0", lambda p: dict(W=p.W.view(-1)[4:]), "16-byte aligned"),
    ("pair_stride 8", "block0", lambda p: dict(pair_stride=8), "does not tile"),
    ("pair_stride 24", "block0", lambda p: dict(pair_stride=24), "does not tile"),
    ("N % (2 pair_stride)", "block0", lambda p: dict(N=96, pair_stride=32), "does not tile"),
    ("mode 3", "block0", lambda p: dict(mode=3), "mode=3"),
    ("mode -1", "block0", lambda p: dict(mode=-1), "mode=-1"),
    ("no segment", "block0", lambda p: dict(segs=[]), "nseg=0"),
    ("segment ld % 4", "block0", lambda p: dict(segs=_seg(p, (0, 64, 0), ld=1166)), "segment 0 destination"),
    ("segments with a gap", "block1", lambda p: dict(segs=_seg(p, (0, 96, 1), (128, 160, 1))), "segments must tile"),
    ("segment not a multiple of 2 pair_stride", "block1", lambda p: dict(segs=_seg(p, (0, 80, 1), (80, 128, 1), (128, 160, 0))), "segments must tile"),
    ("empty segment", "block1", lambda p: dict(segs=_seg(p, (0, 96, 1), (96, 96, 1), (96, 160, 0))), "segments must tile"),
    ("segments short of N", "block1", lambda p: dict(segs=_seg(p, (0, 96, 1), (96, 128, 1))), "segments cover"),
    ("rope without tables", "block1", lambda p: dict(rope_cos=None, rope_sin=None), "rope needs"),
    ("rope_half != pair_stride", "block1", lambda p: dict(rope_half=8), "rope needs"),
    ("rope_half != pair_stride (in-block)", "fold1", lambda p: dict(rope_half=32), "rope needs"),
    ("GeGLU pair_stride != N / 2", "block2", lambda p: dict(pair_stride=16), "geglu needs"),
    ("GeGLU pair_stride != N / 2 (in-block)", "fold2", lambda p: dict(pair_stride=16), "geglu needs"),
    ("w_packed, block-split", "block0", lambda p: dict(w_packed=True), "w_packed needs"),
    ("w_packed, split-K", "splitk", lambda p: dict(w_packed=True), "w_packed needs"),
    ("A beyond 2 GiB", "in0", lambda p: dict(M=2, a_map=(1, 1 << 20, 0)), "A spans"),
    ("trace buffer too small", "in0", lambda p: dict(workspace=p.ws[:8]), "trace buffer"),
    ("in-block K = 512", "in0", lambda p: dict(K=512), "in-block K needs"),
    ("in-block K = 1536", "in0", lambda p: dict(K=1536), "in-block K needs"),
    ("in-block mode 0, N % 128", "in0", lambda p: dict(N=96), "in-block mode 0 needs"),
    ("in-block mode 2, K = 2048", "in2", lambda p: dict(K=2048), "built for K = 1024"),
    ("in-block mode 1, K = 4096", "fold1", lambda p: dict(K=4096, rowsq_in=None, cvec=None), "built for K = 1024"),
    ("folded with mod", "fold2", lambda p: dict(mod=p.mod, mod_ld=3 * 4104, mod_rpb=25), "folded adaRMS form needs"),
    ("folded with a_map", "fold2", lambda p: dict(a_map=(25, 25, 0)), "folded adaRMS form needs"),
    ("folded with mode 0", "in0", lambda p: dict(rowsq_in=p.rowsq, rowsq_parts=3, cvec=p.cvec), "folded adaRMS form needs"),
    ("folded, K = 2048", "fold2", lambda p: dict(K=2048), "folded adaRMS form needs"),
    ("rowsq_parts = 0", "fold2", lambda p: dict(rowsq_parts=0), "folded adaRMS form needs"),
    ("rowsq_parts = 65", "fold1", lambda p: dict(rowsq_parts=65), "folded adaRMS form needs"),
    ("rowsq_ld < M", "fold2", lambda p: dict(rowsq_in=p.rowsq[:, :48].contiguous()), "folded adaRMS form needs"),
    ("cvec misaligned", "fold2", lambda p: dict(cvec=p.cvec[1:]), "folded adaRMS form needs"),
    ("mod with mode 0", "in0", lambda p: dict(mod=p.mod, mod_ld=3 * 4104, mod_rpb=25), "adaRMS prologue needs"),
    ("mod, K = 2048", "ada2", lambda p: dict(K=2048), "adaRMS prologue needs"),
    ("mod_rpb = 0", "ada2", lambda p: dict(mod_rpb=0), "adaRMS prologue needs"),
    ("mod_ld < 2 K", "ada2", lambda p: dict(mod_ld=2044), "adaRMS prologue needs"),
    ("mod_ld % 4", "ada2", lambda p: dict(mod_ld=3 * 4104 + 2), "adaRMS prologue needs"),
    ("mod misaligned", "ada2", lambda p: dict(mod=p.mod[:, 1:]), "adaRMS prologue needs"),
    ("mod with a_map", "ada2", lambda p: dict(a_map=(25, 25, 0)), "adaRMS prologue needs"),
    ("rowsq_out with mode 2", "in2", lambda p: dict(rowsq_out=p.sq_out), "rowsq_out needs"),
    ("rowsq_out_ld < M", "in0", lambda p: dict(rowsq_out=p.sq_out[:, :48].contiguous()), "rowsq_out needs"),
    ("rowsq_out, N = 1152", "in0", lambda p: dict(N=1152, segs=_seg(p, (0, 1152, 0)), rowsq_out=p.sq_out), "rowsq_out needs"),
    ("mod, block-split", "block2", lambda p: dict(mod=p.mod, mod_ld=3 * 4104, mod_rpb=25), "need split_k == -1"),
    ("rowsq_in, block-split", "block2", lambda p: dict(rowsq_in=p.rowsq, rowsq_parts=3, cvec=p.cvec), "need split_k == -1"),
    ("rowsq_out, block-split", "block0", lambda p: dict(rowsq_out=p.sq_out), "need split_k == -1"),
    ("split-K with a gate", "splitk", lambda p: dict(gate=p.gate, gate_rpb=25, gate_ld=1168), "produces raw partial products"),
    ("split-K with a residual", "splitk", lambda p: dict(residual=p.res, ldr=1168), "produces raw partial products"),
    ("split-K with mode 2", "splitk", lambda p: dict(mode=2, pair_stride=32), "produces raw partial products"),
    ("split-K workspace too small", "splitk", lambda p: dict(workspace=p.ws[: 2 * M0 * 64 - 4]), "workspace bytes"),
    ("split-K workspace misaligned", "splitk", lambda p: dict(workspace=p.ws[1 : 2 * M0 * 64 + 1]), "workspace bytes"),
]


@pytest.fixture(scope="module")
def pool():
    return Pool()


@pytest.mark.parametrize("name,form,change,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_descriptor(ops, pool, name, form, change, message):
    """Every KAI0_REQUIRE of kai0_gemm_skinny_bf16 / skinny_inblock that ops.skinny_gemm can reach (a null A, W or destination and
    more than three segments cannot get through the wrapper): Kai0HipError with that check's message, nothing launched — the output and
    the workspace keep their sentinel."""
    from kai0_amd._lib import Kai0HipError

    kw = dict(_forms(pool)[form])
    kw.update(change(pool))
    A, W = kw.pop("A", pool.A), kw.pop("W", pool.W)
    with pytest.raises(Kai0HipError, match=message):
        ops.skinny_gemm(A, W, **kw)
    torch.cuda.synchronize()
    assert bool((pool.out == R.SENTINEL).all()) and bool((pool.ws == R.SENTINEL).all()) and bool((pool.sq_out == R.SENTINEL).all()), name


def test_every_form_of_the_refusal_table_is_accepted_unchanged(ops, pool):
    """The starting points themselves launch: a refusal above is caused by the one change it names."""
    for form, kw in _forms(pool).items():
        ops.skinny_gemm(pool.A, pool.W, **kw)
    torch.cuda.synchronize()
    pool.out.fill_(R.SENTINEL)
    pool.ws.fill_(R.SENTINEL)
