"""kai0_gemm_bf16's 256 x 256 tile family — the NT quadrant schedule, the TN 32-deep ring, the plain two-stage loop of NN / TT and the
persistent NT kernel — held to the per-element float64 bound of tests/gemm_refs.py at ragged edges, K tails, split-K slices shorter
than the pipeline (and empty ones), two-level batch strides and every linear epilogue.

The library picks these tiles only for launches of >= 160 tiles of 256 x 256 (kai0hip.h, kai0_gemm_plan_t).  Batch entries count, so
160 entries of one small ragged problem reach them with every block a ragged tile; every case first asks `ops.gemm_plan` which kernel
its descriptor gets, so a change of the dispatch rule cannot quietly send these cases to the 128 x 128 tile.

Outputs are pre-filled with a sentinel and everything outside the [M, N] windows — row padding up to ldc, the gaps between batch
entries — must come back unchanged.  Inputs: A ~ N(0, 1), B ~ 0.05 N(0, 1), seeded, asymmetric."""

import functools

import pytest
import torch

import gemm_refs as R

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOOP = {"NT": "quadrant", "TN": "ring", "NN": "plain2", "TT": "plain2"}
WORST = {}  # case family -> worst err / bound seen (printed per test; profiles/HISTORY.md records a run)


@pytest.fixture(scope="module")
def ops():
    from kai0_amd import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _rnd_cpu(n, seed, scale, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dtype)


def rnd(n, seed, scale=1.0, dtype=BF16):
    return _rnd_cpu(n, seed, scale, dtype).to(dev())


def note(family, what, w):
    WORST[family] = max(WORST.get(family, 0.0), w)
    print(f"[{family}] {what}: worst err / bound {w:.3f} (family so far {WORST[family]:.3f})")


class Problem:
    """One batched GEMM on padded storage: leading dimensions 8 past the row length, inner batch stride 16 past an entry, outer stride
    24 past `inner` entries — so sX1 != inner * sX2 and a kernel that swaps z1 and z2, or uses another operand's stride, reads or
    writes the wrong entry."""

    def __init__(self, lay, M, N, K, outer=1, inner=1, ldc=None):
        self.lay, self.M, self.N, self.K, self.outer, self.inner = lay, M, N, K, outer, inner
        ar, ac = (M, K) if lay[0] == "N" else (K, M)
        br, bc = (N, K) if lay[1] == "T" else (K, N)
        self.lda, self.ldb = (ac + 7) // 8 * 8 + 8, (bc + 7) // 8 * 8 + 8
        self.ldc = ldc if ldc is not None else (N + 7) // 8 * 8 + 8
        self.sA, self.a_len = self._strides(ar * self.lda)
        self.sB, self.b_len = self._strides(br * self.ldb)
        self.sC, self.c_len = self._strides(M * self.ldc)
        self.A, self.B = rnd(self.a_len, 1), rnd(self.b_len, 2, 0.05)
        self.a, self.b = R.operands(self.A, self.B, lay, M, N, K, self.lda, self.ldb, outer=outer, inner=inner, sA=self.sA, sB=self.sB)

    def _strides(self, entry):
        s2 = entry + 16
        s1 = self.inner * s2 + 24
        return (s1, s2), self.outer * s1

    def c_like(self, seed=None, dtype=BF16):
        """Storage laid out like C: random (an operand addressed like C) or sentinel-filled (an output)."""
        if seed is None:
            return torch.full((self.c_len,), R.SENTINEL, dtype=dtype, device=dev())
        return rnd(self.c_len, seed, dtype=dtype)

    def window(self, store, ld=None, strides=None, cols=None):
        s = strides or self.sC
        return R.view(store, self.M, cols or self.N, ld or self.ldc, outer=self.outer, inner=self.inner, s1=s[0], s2=s[1])

    def kw(self, **extra):
        kw = dict(M=self.M, N=self.N, K=self.K, lda=self.lda, ldb=self.ldb, ldc=self.ldc, batch=self.outer * self.inner,
                  batch_inner=self.inner, sA=self.sA, sB=self.sB, sC=self.sC, **R.layout_flags(self.lay))
        kw.update(extra)
        return kw

    def assert_padding_untouched(self, store, what, cols=None):
        """Everything outside the [M, cols] windows still holds the sentinel `store` was filled with."""
        masked = store.clone()
        self.window(masked, cols=cols).fill_(R.SENTINEL)
        assert torch.equal(masked, torch.full_like(store, R.SENTINEL)), f"{what}: a write outside the [M, N] windows"


def expect_plan(ops, A, B, out, kw, *, tile=256, loop=None, **fields):
    plan = ops.gemm_plan(A, B, out, **kw)
    want = dict(tile=tile, **fields)
    if loop is not None:
        want["loop"] = loop
    got = {k: plan[k] for k in want}
    assert got == want, f"dispatch: expected {want}, the library plans {plan}"
    return plan


def run(ops, pr, family, what, *, store=None, plan=None, ref_epi=None, **kw):
    """Plan check, launch into a sentinel-filled (or given) store, every element against the f64 bound, padding check."""
    out = pr.c_like(dtype=F32 if (ref_epi or {}).get("out_f32") else BF16) if store is None else store
    args = pr.kw(**kw)
    expect_plan(ops, pr.A, pr.B, out, args, **(plan or dict(loop=LOOP[pr.lay])))
    ref, bound = R.reference(pr.a, pr.b, **(ref_epi or {}))
    ops.gemm(pr.A, pr.B, out, **args)
    torch.cuda.synchronize()
    note(family, what, R.assert_within(pr.window(out), ref, bound, what))
    return out


# ------------------------------------------------------------------------------------------------ a. plain product
PLAIN = [(lay, M, N, K, o, i) for lay in ("NT", "NN", "TN", "TT")
         for (M, N, K, o, i) in [(256, 256, 256, 20, 8), (200, 136, 264, 20, 8), (8, 8, 320, 20, 8), (264, 520, 328, 9, 3)]]
PLAIN += [("TN", 200, 136, 263, 20, 8), ("TN", 200, 136, 1000, 20, 8)]


@pytest.mark.parametrize("lay,M,N,K,outer,inner", PLAIN)
def test_plain_product(ops, lay, M, N, K, outer, inner):
    pr = Problem(lay, M, N, K, outer, inner)
    out = run(ops, pr, "a", f"{lay} {M}x{N}x{K} x {outer}*{inner}", plan=dict(loop=LOOP[lay], tiles_m=(M + 255) // 256, tiles_n=(N + 255) // 256, k_chunk=K))
    pr.assert_padding_untouched(out, f"{lay} {M}x{N}x{K}")


def test_plain_product_n_not_multiple_of_8(ops):
    """N = 20 with ldc = 24 (NT only): columns 20..23 of every row come out as exact zeros (kai0hip.h), nothing past them is touched."""
    pr = Problem("NT", 200, 20, 264, 20, 8, ldc=24)
    out = run(ops, pr, "a", "NT 200x20x264, ldc 24")
    assert float(pr.window(out, cols=24)[..., 20:].abs().max()) == 0.0
    pr.assert_padding_untouched(out, "N = 20", cols=24)


# ------------------------------------------------------------------------------------------------ b. split-K
def _bias_res(pr, seed=3):
    """bias + residual on its own leading dimension and batch strides (neither is C's)."""
    ldr = pr.ldc + 8
    s2 = pr.M * ldr + 32
    sR = (pr.inner * s2 + 40, s2)
    res = rnd(pr.outer * sR[0], seed + 1)
    bias = rnd(pr.N, seed)
    return dict(bias=bias, residual=res, ldr=ldr, sR=sR), dict(bias=bias, residual=pr.window(res, ld=ldr, strides=sR))


SPLIT_4, SPLIT_27 = (200, 136, 264, 5, 8, 4, 128), (264, 520, 1000, 1, 1, 27, 64)
SPLITS = [(lay, *shape, epi) for lay in ("NT", "TN", "NN") for shape in (SPLIT_4, SPLIT_27) for epi in ("plain", "bias_res")]
SPLITS.append(("NT", *SPLIT_4, "out_f32"))


@pytest.mark.parametrize("lay,M,N,K,outer,inner,split,k_chunk,epi", SPLITS)
def test_split_k(ops, lay, M, N, K, outer, inner, split, k_chunk, epi):
    """(200, 136, 264) / 4: slices of 128, 128, 8 and an EMPTY one, summed by the reduction's unrolled form (split <= 8);
    (264, 520, 1000) / 27: 16 live slices of 64 (the last of 40: two ring sub-tiles per slice with three in flight) and 11 empty ones,
    summed by its loop form (split > 8).  Plain, with bias + residual through the reduction, and one f32 output."""
    pr = Problem(lay, M, N, K, outer, inner)
    kw, ref_epi = ({}, {}) if epi != "bias_res" else _bias_res(pr)
    if epi == "out_f32":
        ref_epi = dict(out_f32=True)
    out = run(ops, pr, "b", f"split {lay} {M}x{N}x{K}/{split} {epi}", plan=dict(loop=LOOP[lay], k_chunk=k_chunk), ref_epi=ref_epi, split_k=split, **kw)
    pr.assert_padding_untouched(out, f"split {lay} {epi}")


# ------------------------------------------------------------------------------------------------ c. linear epilogues
def _gate(pr):
    rpb = 8
    gate_ld = pr.N + 16
    g = rnd((pr.M // rpb) * gate_ld, 7)
    return dict(gate=g, gate_rpb=rpb, gate_ld=gate_ld), dict(gate=g.view(pr.M // rpb, gate_ld)[:, : pr.N].repeat_interleave(rpb, 0))


EPILOGUES = ["bias", "bias_f32", "residual", "gate", "scale", "accumulate", "accumulate_bias_residual", "out_f32"]


@pytest.mark.parametrize("lay,form", [("NT", f) for f in EPILOGUES] + [(lay, f) for lay in ("TN", "NN") for f in ("residual", "accumulate")])
def test_linear_epilogues(ops, lay, form):
    """Every linear epilogue at (200, 136, 264) x 160 under general_epilogue 0 and 1: both within the bound, and the same bits."""
    pr = Problem(lay, 200, 136, 264, 20, 8)
    kw, ref_epi = {}, {}
    if form in ("bias", "bias_f32"):
        b = rnd(pr.N, 3, dtype=F32 if form == "bias_f32" else BF16)
        kw, ref_epi = dict(bias=b), dict(bias=b)
    elif form == "residual":
        kw, ref_epi = _bias_res(pr)
        kw.pop("bias"), ref_epi.pop("bias")
    elif form == "gate":
        kw, ref_epi = _gate(pr)
    elif form == "scale":
        kw, ref_epi = dict(scale=0.3), dict(scale=0.3)
    elif form == "accumulate_bias_residual":
        kw, ref_epi = _bias_res(pr)
    elif form == "out_f32":
        ref_epi = dict(out_f32=True)
    outs = []
    for general in (0, 1):
        store = None
        if form.startswith("accumulate"):  # C prefilled: random inside the windows, the sentinel around them
            kw["accumulate"] = True
            store = pr.c_like()
            pr.window(store).copy_(pr.window(pr.c_like(seed=9)))
            ref_epi["c_old"] = pr.window(store).clone()
        with ops.gemm_tuning(general_epilogue=general):
            simple = general == 0 and form not in ("gate", "scale", "out_f32")
            outs.append(run(ops, pr, "c", f"{lay} {form} general_epilogue={general}", store=store, ref_epi=ref_epi,
                            plan=dict(loop=LOOP[lay], simple_epilogue=simple), **kw))
        pr.assert_padding_untouched(outs[-1], f"{lay} {form}")
    assert torch.equal(outs[0], outs[1]), f"{lay} {form}: the fast and the general epilogue differ"


# ------------------------------------------------------------------------------------------------ d. what batch > 1 excludes
BM, BN, BK_ = 2312, 4104, 264  # the smallest single launch of >= 160 tiles here: 10 x 17, 8-wide remnants on both edges


@functools.lru_cache(maxsize=None)
def _single(lay="NT"):
    """The one-entry problem of family d and its f64 reference, computed once."""
    pr = Problem(lay, BM, BN, BK_)
    return pr, R.reference(pr.a, pr.b)


def test_routed_column_segments(ops):
    """Three destinations with their own leading dimensions; a boundary inside a 256-column tile and one on an 8-column group."""
    pr, (ref, bound) = _single()
    begins, ends = (0, 2056, 3080), (2056, 3080, BN)
    dst = [torch.full((BM, e - b + 8 * (i + 1)), R.SENTINEL, dtype=BF16, device=dev()) for i, (b, e) in enumerate(zip(begins, ends))]
    out = pr.c_like()
    kw = pr.kw(segs=[(d, d.shape[1], b) for d, b in zip(dst, begins)])
    for general in (0, 1):
        with ops.gemm_tuning(general_epilogue=general):
            expect_plan(ops, pr.A, pr.B, out, kw, loop="quadrant", tiles_m=10, tiles_n=17)
            ops.gemm(pr.A, pr.B, out, **kw)
        for d, b, e in zip(dst, begins, ends):
            note("d", f"segment [{b}, {e})", R.assert_within(d[:, : e - b], ref[0, 0, :, b:e], bound[0, 0, :, b:e], f"segment at {b}"))
            assert bool((d[:, e - b :] == R.SENTINEL).all()), f"segment at {b}: padding columns written"
            d[:, : e - b] = R.SENTINEL
        assert bool((out == R.SENTINEL).all()), "routed launch wrote C"


def test_geglu_pair(ops):
    """act 6 on the quadrant schedule, 10 x 17 tiles with a ragged last row block and a last tile of 32 output columns: the
    pre-activations g and u against the f64 product (plain bound), h against bf16(gelu_tanh(g)) * u restated in f64 from the kernel's
    own g and u — the rounding points of test_gemm_geglu_pair_equals_gate_gemm_plus_up_gemm.  h's bound: the bf16 rounding of the
    gelu and of h (2^-8 each, relative) plus the fast gelu's error |g| (2e-7 + 8 * 2^-23) (common.h: 2e-7 absolute on the sigmoid; a
    handful of f32 operations)."""
    M, Fd, K = BM, 2080, BK_
    pr = Problem("NT", M, Fd, K)
    wu = rnd(pr.b_len, 5, 0.05)
    h, g, u = pr.c_like(), pr.c_like(), pr.c_like()
    kw = pr.kw(act=6, B2=wu, pre_out=g, pre_out2=u)
    expect_plan(ops, pr.A, pr.B, h, kw, loop="quadrant", tiles_m=10, tiles_n=17)
    ops.gemm(pr.A, pr.B, h, **kw)
    for got, w, name in ((g, pr.B, "g"), (u, wu, "u")):
        a, b = R.operands(pr.A, w, "NT", M, Fd, K, pr.lda, pr.ldb)
        note("d", f"pair {name}", R.assert_within(pr.window(got), *R.reference(a, b), f"pair {name}"))
        pr.assert_padding_untouched(got, f"pair {name}")
    g64, u64 = pr.window(g).to(F64), pr.window(u).to(F64)
    ge = torch.nn.functional.gelu(g64, approximate="tanh")
    eg = g64.abs() * (2e-7 + 8 * R.U32)
    e1 = u64.abs() * (eg + R.UBF * (ge.abs() + eg))
    ref = ge * u64
    e1 = e1 + R.U32 * ref.abs()  # (the f32 multiply)
    note("d", "pair h", R.assert_within(pr.window(h), ref, e1 + R.UBF * (ref.abs() + e1) + R.TINY, "pair h"))
    pr.assert_padding_untouched(h, "pair h")


def test_output_row_map(ops):
    """c_map: 8 groups of 289 rows into a buffer of 304 rows per group, from row 8 — the rows around them stay untouched."""
    pr, (ref, bound) = _single()
    rpb, S_ld, row0 = 289, 304, 8
    buf = torch.full((8, S_ld, pr.ldc), R.SENTINEL, dtype=BF16, device=dev())
    kw = pr.kw(c_map=(rpb, S_ld, row0))
    expect_plan(ops, pr.A, pr.B, buf, kw, loop="quadrant", simple_epilogue=False)
    ops.gemm(pr.A, pr.B, buf, **kw)
    note("d", "c_map", R.assert_within(buf[:, row0 : row0 + rpb, :BN].reshape(1, 1, BM, BN), ref, bound, "c_map"))
    buf[:, row0 : row0 + rpb, :BN] = R.SENTINEL
    assert bool((buf == R.SENTINEL).all()), "c_map: a write outside the mapped rows"


def test_input_row_map_on_nt_rows(ops):
    """a_map: the same rows read out of a padded [8][304] row buffer whose other rows hold NaN-free garbage of another scale."""
    pr, (ref, bound) = _single()
    rpb, S_ld, row0 = 289, 304, 8
    abuf = rnd(8 * S_ld * pr.lda, 11, 40.0).view(8, S_ld, pr.lda)
    abuf[:, row0 : row0 + rpb] = pr.A[: BM * pr.lda].view(8, rpb, pr.lda)
    out = pr.c_like()
    kw = pr.kw(a_map=(rpb, S_ld, row0))
    expect_plan(ops, abuf, pr.B, out, kw, loop="quadrant")
    ops.gemm(abuf, pr.B, out, **kw)
    note("d", "a_map (NT rows)", R.assert_within(pr.window(out), ref, bound, "a_map on NT rows"))
    pr.assert_padding_untouched(out, "a_map")


def test_input_row_map_on_tn_contraction_rows(ops):
    """TN with the CONTRACTION rows of A remapped (8 groups of 33 k-rows out of 40), split in two so that the slices are 192 and 72."""
    pr, (ref, bound) = _single("TN")
    rpb, S_ld, row0 = 33, 40, 3
    abuf = rnd(8 * S_ld * pr.lda, 11, 40.0).view(8, S_ld, pr.lda)
    abuf[:, row0 : row0 + rpb] = pr.A[: BK_ * pr.lda].view(8, rpb, pr.lda)
    out = pr.c_like()
    kw = pr.kw(a_map=(rpb, S_ld, row0), split_k=2)
    expect_plan(ops, abuf, pr.B, out, kw, loop="ring", k_chunk=192)
    ops.gemm(abuf, pr.B, out, **kw)
    note("d", "a_map (TN contraction rows)", R.assert_within(pr.window(out), ref, bound, "a_map on TN contraction rows"))
    pr.assert_padding_untouched(out, "a_map TN")


# ------------------------------------------------------------------------------------------------ e. nonlinear epilogues
def _act_launch(ops, pr, act, batch):
    """Outputs and arguments for the first `batch` entries of the 160-entry data with activation `act`."""
    outs = [pr.c_like()]
    kw = dict(act=act)
    if act in (1, 2, 3):
        outs.append(pr.c_like())
        kw["pre_out"] = outs[1]
    if act == 1:
        kw["bias"] = rnd(pr.N, 3)
    if act in (2, 3, 5):
        kw["aux1"] = pr.c_like(seed=6)
    if act == 3:
        kw["aux2"] = pr.c_like(seed=7)
    if act == 4:
        kw.update(aux1=(pr.c_like(seed=6).float().abs() * 0.1).to(BF16), rowvec=rnd(pr.outer * pr.inner * pr.M, 8, dtype=F32),
                  rv=(pr.inner * pr.M, pr.M, 1), scale=0.125)
    args = pr.kw(**kw)
    args["batch"] = batch
    return outs, args


def test_nonlinear_epilogues_equal_the_128_tile_bit_for_bit(ops):
    """Acts 1-5 use fast exp / rcp, so no bound is derived for them; the 128 x 128 tile is the yardstick instead.  160 entries of
    (200, 136, 264) run the 256 x 256 quadrant kernel; the first 159 entries of the same data, launched as batch 159, run the
    128 x 128 kernel.

    Do the two tiles sum in the same order?  Yes.  Every K loop of csrc/gemm_bf16.hip feeds each accumulator the same instruction,
    mfma_f32_16x16x32_bf16, once per 32 k in ascending k: the plain loop runs ks = 0, 1 inside each 64-deep K-tile, the quadrant
    schedule's quad() runs ks = 0, 1 of tile t before tile t + 1, the ring takes one 32-deep sub-tile per step.  The fragments come
    from the same load_frag in all of them (lane group g holds k chunk ks * 4 + g), so the k that meet inside one MFMA are the same
    too, and out-of-range k are zero-filled in both.  The epilogue code is shared.  Hence act 0 is checked first to give the same
    bits, and then every act must: C and pre_out of entries 0..158 equal bit for bit.  Entry 159 (not in the 128-tile launch) is
    checked for written and finite.

    Not covered here: pre_out2.  Only act 6 writes it, and the library refuses act 6 with batch > 1, so no 160-against-159 launch
    of it exists; test_geglu_pair holds pre_out2 (u) of the 256 x 256 kernel to the f64 bound instead, on one launch of 170 tiles."""
    pr = Problem("NT", 200, 136, 264, 20, 8)
    for act in (0, 1, 2, 3, 4, 5):
        big, args = _act_launch(ops, pr, act, 160)
        expect_plan(ops, pr.A, pr.B, big[0], args, loop="quadrant")
        ops.gemm(pr.A, pr.B, big[0], **args)
        small, args = _act_launch(ops, pr, act, 159)  # (batch_inner stays 8: z = 0..158 are the same entries)
        expect_plan(ops, pr.A, pr.B, small[0], args, tile=128)
        ops.gemm(pr.A, pr.B, small[0], **args)
        torch.cuda.synchronize()
        for got, want, name in zip(big, small, ("C", "pre_out")):
            g, w = pr.window(got).reshape(160, pr.M, pr.N), pr.window(want).reshape(160, pr.M, pr.N)
            assert torch.equal(g[:159], w[:159]), f"act {act} {name}: the 256 x 256 and the 128 x 128 tile differ in {int((g[:159] != w[:159]).sum())} elements"
            assert bool(torch.isfinite(g[159].float()).all()) and bool((g[159] != R.SENTINEL).all()), f"act {act} {name}: entry 159"
            assert bool((w[159] == R.SENTINEL).all())
            pr.assert_padding_untouched(got, f"act {act} {name}")
        if act == 0:  # and the yardstick itself is right
            ref, bound = R.reference(pr.a, pr.b)
            keep = pr.window(small[0]).reshape(160, pr.M, pr.N)[:159]
            note("e", "act 0, 128 x 128 tile", R.assert_within(keep, ref.reshape(160, pr.M, pr.N)[:159], bound.reshape(160, pr.M, pr.N)[:159], "128 tile"))


# ------------------------------------------------------------------------------------------------ f. dispatch boundary
def test_dispatch_boundaries(ops):
    """kai0_gemm_plan either side of every threshold of the selection.  Plans only: nothing is launched, the operands are dummies."""
    t = torch.zeros(64, dtype=BF16, device=dev())

    def plan(M, N, K, lay="NT", **kw):
        args = dict(M=M, N=N, K=K, ldc=N, lda=(K if lay[0] == "N" else M), ldb=(K if lay[1] == "T" else N), **R.layout_flags(lay))
        args.update(kw)
        return ops.gemm_plan(t, t, t, **args)

    def batched(n, K=264, **kw):
        return plan(200, 136, K, batch=n, sA=(200 * K, 0), sB=(136 * K, 0), sC=(200 * 136, 0), **kw)

    with ops.gemm_tuning(persist=0, small_w8=0, general_epilogue=0):
        # 160 tiles of 256 x 256, batch entries and split-K slices counted
        assert batched(159)["tile"] == 128 and batched(160)["tile"] == 256
        assert batched(39, split_k=4)["tile"] == 128 and batched(40, split_k=4)["tile"] == 256
        assert plan(2304, 4104, 264)["tile"] == 128 and plan(2312, 4104, 264)["tile"] == 256  # 9 x 17 = 153 | 10 x 17 = 170
        # K >= 256 (the problem's K, not the slice's)
        assert batched(160, K=248)["tile"] == 128 and batched(160, K=256)["tile"] == 256
        assert batched(40, K=256, split_k=4) == dict(tile=256, waves=8, loop="quadrant", tiles_m=1, tiles_n=1, k_chunk=64, simple_epilogue=False)
        # the three 256 layouts
        for lay, loop in LOOP.items():
            p = plan(2312, 4104, 264, lay)
            assert (p["tile"], p["waves"], p["loop"], p["tiles_m"], p["tiles_n"]) == (256, 8, loop, 10, 17), (lay, p)
        # act 7 (RoPE epilogue) always runs the 128-column tiles
        M, N = 2560, 4352
        cs = torch.zeros(M, 128, dtype=BF16, device=dev())
        assert plan(M, N, 264)["tile"] == 256
        p7 = plan(M, N, 264, act=7, rope=(cs, cs, 128, 4096))
        assert (p7["tile"], p7["tiles_m"], p7["tiles_n"]) == (128, 20, 34), p7
        # 128 x 128: four stages when the grid is at most one block per CU (<= 256 blocks) and a slice is >= 256 deep; eight waves
        # then for K-contiguous operands with act 0 / 1
        assert plan(2048, 2048, 256) == dict(tile=128, waves=8, loop="plain4", tiles_m=16, tiles_n=16, k_chunk=256, simple_epilogue=False)
        assert (plan(2048, 2048, 248)["waves"], plan(2048, 2048, 248)["loop"]) == (4, "plain2")
        assert (plan(2048, 2176, 256)["waves"], plan(2048, 2176, 256)["loop"]) == (4, "plain2")  # 272 blocks
        assert (plan(2048, 2048, 256, "NN")["waves"], plan(2048, 2048, 256, "NN")["loop"]) == (4, "plain4")
        p = plan(1024, 512, 1000, split_k=4)  # 32 blocks x 4, slices of 256
        assert (p["waves"], p["loop"], p["k_chunk"]) == (8, "plain4", 256), p
        p = plan(1024, 512, 1000, split_k=5)  # slices of 256 (200 rounded up to the 64-deep tile): 4 live, 1 empty
        assert (p["loop"], p["k_chunk"]) == ("plain4", 256), p
        assert plan(1024, 512, 1000, split_k=8)["loop"] == "plain2"  # slices of 128
        # persistent NT kernel: one entry, no split, >= 2048 tiles and N >= 8192 or K >= 8192
        assert plan(16384, 8192, 256)["loop"] == "persistent" and plan(16384, 7936, 256)["loop"] == "quadrant"  # 2048 | 1984 tiles
        assert plan(32768, 4096, 256)["loop"] == "quadrant" and plan(32768, 4096, 8192)["loop"] == "persistent"  # 2048 tiles, the N / K rule
        assert plan(16384, 8192, 256, a_map=(16384, 16384, 0))["loop"] == "quadrant"
        assert plan(16384, 8192, 264, "TN")["loop"] == "ring"
        # the simple epilogue: 256 x 256, act 0 / 1, no gate / scale / f32 output / output row map / split
        assert plan(2312, 4104, 264)["simple_epilogue"] and plan(2312, 4104, 264, bias=t, residual=t, ldr=4104, accumulate=True)["simple_epilogue"]
        assert not plan(2312, 4104, 264, gate=t, gate_rpb=8, gate_ld=4104)["simple_epilogue"]
        assert not plan(2312, 4104, 264, scale=0.5)["simple_epilogue"] and not plan(2312, 4104, 264, c_map=(289, 304, 8))["simple_epilogue"]
        assert not plan(2304, 4104, 264)["simple_epilogue"]  # (128 x 128)
    with ops.gemm_tuning(general_epilogue=1):
        assert not plan(2312, 4104, 264)["simple_epilogue"]
    with ops.gemm_tuning(persist=1):
        assert plan(16384, 8192, 256)["loop"] == "quadrant"
    with ops.gemm_tuning(persist=2):  # every eligible NT launch of >= 512 tiles
        assert plan(4096, 8192, 256)["loop"] == "persistent" and plan(4096, 7936, 256)["loop"] == "quadrant"
    with ops.gemm_tuning(small_w8=1):
        assert (plan(2048, 2048, 256)["waves"], plan(2048, 2048, 256)["loop"]) == (4, "plain4")
    with ops.gemm_tuning(small_w8=2):
        assert (plan(2048, 2176, 256)["waves"], plan(2048, 2176, 256)["loop"]) == (8, "plain4")
    from kai0_amd._lib import Kai0HipError

    with pytest.raises(Kai0HipError, match="multiples of 8"):  # the launch's validation, not a copy of it
        plan(256, 256, 256, lda=260)
