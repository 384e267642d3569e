"""Float64 references, per-element error bounds and input builders for kai0_gemm_skinny_bf16 (csrc/skinny.hip), after the rounding
points of include/kai0hip.h.  A plain helper module like tests/gemm_refs.py and tests/streaming_refs.py, built out of those two:
nothing here touches the HIP library, everything runs on whichever device its inputs live on.

One formula per form.  Every form is written ONCE as a function of the accumulator it is handed:

  f64 accumulator + error  the reference.  No intermediate rounding; the header's rounding points are accounted for in the bound that
                           is carried alongside the value as the chain (x, e) of gemm_refs.Chain.
  f32 accumulator, no error  the emulation tests/test_skinny_refs_cpu.py holds against the bound: f32 arithmetic with the header's bf16
                           rounding points (and the fast GELU of csrc/common.h).  The kernels are never used to choose a constant.

The chain (x, e) = (exact value, bound on |computed - exact|), U32 = 2^-23, UBF = 2^-8 as in gemm_refs:

  accumulation  x = sum_k a w, e = K * U32 * (|A| |W|): the argument of gemm_refs (any order and grouping of K f32 addends, twice
                Higham's (K - 1) 2^-24 sum|terms|).  Independent of the order, so it covers the 4 / 8 / 16 wave partials that meet
                in LDS and the split-K slices.  With split_k > 1 the kernel stores the raw f32 partial of slice s: that one is held to
                (K / split_k) * U32 * T_s, T_s = |A_s| |W_s| over the slice.
  folded form   out = v * rstd + cvec[n], rstd = rsqrt(sum_p rowsq_in[p][row] / K + eps) from the partials AS GIVEN (the reference
                takes the same f32 partials and adds them in f64).  The f32 sum of `parts` non-negative partials is off by at most
                (parts - 1) 2^-24 relative, the divide and the add of eps by 2^-24 each; rsqrt halves the relative error of its
                argument and adds one ulp of its own (2^-23); the multiply adds 2^-24.  In units of U32 that is at most
                (parts + 1) / 4 + 1 + 1 / 2 <= parts + 4, so
                    e <- e * rstd + (parts + 4) * U32 * |v rstd|,  then  + U32 * |result|  for the add of cvec.
  linear        bf16 -> * gate -> + residual: gemm_refs.epilogue, unchanged.
  RoPE          out1 = bf16(bf16(x1 c) + bf16(-x2 s)), out2 = bf16(bf16(x2 c) + bf16(x1 s)) on x = bf16(accumulator): Chain.round_bf16,
                Chain.mul by the table value, the sum of two chains (their errors add, + U32 * |sum| for the f32 add), round_bf16.
                The cos / sin tables are INPUTS of the launch (f32 tensors holding bf16-rounded values, built by the test in torch),
                so no libm difference enters.
  GeGLU         h = bf16(bf16(gelu_tanh(bf16 g)) * bf16 u).  After the roundings of g and u:
                    e_gelu = L * e_g + |g| * (SIG_ERR + 8 * U32)
                (L = 1.13 >= sup |gelu_tanh'| = 1.12899..., recomputed on a grid by the CPU test; the second term is the allowance of
                tests/test_gemm_big_tile_gpu.py::test_geglu_pair for the fast GELU of common.h: 2e-7 absolute on the sigmoid, a handful
                of f32 operations), round_bf16, the product rule |u| e_gelu + (|gelu| + e_gelu) e_u + U32 |ref|, round_bf16.
  rowsq_out     rowsq_out[tile][row] against the f64 sum of squares of the 16 bf16 values THE LAUNCH ITSELF STORED in that column tile
                (squares of bf16 values are exact in f32; 15 f32 additions): bound 16 * U32 * sum + TINY.
  adaRMS prologue (`mod`)   y = bf16((x * rstd) * (1 + scale) + shift) feeds the MFMAs.  A generic input would put a whole bf16 ulp
                of error on each of the K = 1024 operands and the bound would mean nothing, so `exact_ada_inputs` builds inputs whose
                prologue is exact: every group of 8 elements of a row is a random permutation of {2, 1, 1, 1, 1/2, 1/2, 1/2, 1/2}
                with random signs, times a per-row 2^j, j in [-2, 2] — the mean square of the row is exactly 4^j — and
                scale in {-4 .. 8} / 8, shift in {-16 .. 16} / 16 per column and batch entry.  With x^ = x / 2^j in +-{2, 1, 1/2}
                every exact y = x^ (1 + scale) + shift is a multiple of 1/16 of magnitude <= 5: at most 7 significant bits, a bf16
                value.  The kernel's rstd = rsqrt(4^j + eps) differs from 2^-j by eps / (2 * 4^j) <= 8e-6 relative (eps = 1e-6), far
                inside half a bf16 ulp, so the bf16 rounding of an f32 evaluation lands back ON the exact y wherever y != 0
                (tests/test_skinny_refs_cpu.py, M = 130, K = 1024: every non-zero y bit for bit; the 2551 elements whose exact y is 0
                come out at <= 8e-6, 0.47 of e_y).  Where the exact y is 0 the two terms cancel and
                what is left is the eps term and the f32 roundings: there
                    e_y = (eps / (2 * meansq) + 4 * U32) * (|x^| (1 + |scale|) + |shift|),
                elsewhere e_y = 0.  The reference multiplies the exact y; sum_k e_y |W| is added to the accumulation term (and e_y to
                |A| inside it).

`gemm_refs.assert_within` holds EVERY element to the bound; no share of the elements is exempt.

Input builders: outputs are sentinel-filled with 8 columns of padding, every operand sits in padded storage whose padding holds NaN
— the rows of A outside the `a_map` windows, the columns K .. K + 8 of A and W, the residual's rows outside the `c_map` windows,
the gate's and the modulation's neighbours in their strided parents, the columns >= M of rowsq_in — so a launch that reads what
it must not read returns a non-finite value, which counts as outside the bound.
"""

import torch
import torch.nn.functional as Fn

import gemm_refs as G
import streaming_refs as S
from gemm_refs import BF16, F32, F64, SENTINEL, TINY, U32, UBF, Chain, assert_within, worst  # noqa: F401  (re-exported)
from streaming_refs import SIG_ERR, rmsnorm_fwd

L_GELU = 1.13  # >= sup |gelu_tanh'| (1.128993 at x = 1.4185)
NAN = float("nan")
EPS = 1e-6

# ------------------------------------------------------------------------------------------------ the cases of both test files
# a. in-block mode 0: (M, a_map = (a_rpb, S_ld, row0) or None).  rpb = 1 takes the division branch of the staged A-tile load, rpb = 2,
# 3, 50, 51 its one-step wrap; M = 1, 5, 17, 50, 102, 130 end on a ragged 16-row tile.
MODE0_MAPS = [(1, None), (5, (1, 3, 2)), (16, None), (17, (3, 8, 1)), (50, (50, 72, 11)), (102, (51, 72, 11)), (130, (2, 8, 4))]
MODE0_K = (1024, 2048, 4096)
MODE0_N = (128, 384)
# b. folded q|k|v: rows of two entries share a 16-row tile at Hs = 51 and Hs = 7
QKV_HEADS = [(2, 256), (3, 32)]
QKV_BATCH = [(1, 1), (1, 16), (1, 17), (1, 50), (2, 51), (3, 7), (2, 64)]
QKV_PARTS = (1, 3, 64)
# c. folded gate|up + GeGLU
GEGLU_CASES = [(F, M) for F in (48, 272) for M in (1, 50, 64, 65, 102)] + [(4096, 50)]
GEGLU_PARTS = (1, 64)
# d. adaRMS prologue: (B, rpb, rows missing from the last entry)
ADA_CASES = [(1, 50, 0), (2, 51, 0), (3, 7, 0), (2, 16, 0), (2, 17, 0), (1, 64, 0), (2, 65, 0), (2, 17, 3), (2, 65, 3)]
# e. block-split kernels and the plain in-block modes 1 / 2
SPLIT_M = (1, 63, 64, 65, 129)
K_BLK = (512, 1024)


# ------------------------------------------------------------------------------------------------ inputs
def rnd(*shape, seed, scale=1.0, dtype=BF16, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(device)


def row_index(M, rmap, device="cpu"):
    """Storage row of logical row r under a row map (rpb, bs, off) of kai0hip.h: (r / rpb) * bs + r % rpb + off; None: identity."""
    r = torch.arange(M, device=device)
    if not rmap:
        return r
    rpb, bs, off = rmap
    return (r // rpb) * bs + r % rpb + off


def map_rows(M, rmap):
    """Rows of the storage a row map addresses: whole entries of `bs` rows."""
    if not rmap:
        return M
    rpb, bs, off = rmap
    assert off + rpb <= bs
    return (M + rpb - 1) // rpb * bs


def padded(x, rmap=None, pad=8, fill=NAN):
    """x [M][W] -> storage [rows][W + pad] holding `fill` everywhere but on the mapped rows' first W columns."""
    M, W = x.shape
    st = torch.full((map_rows(M, rmap), W + pad), fill, dtype=x.dtype, device=x.device)
    st[row_index(M, rmap, x.device), :W] = x
    return st


def sentinel_out(rows, width, pad=8, dtype=BF16, device="cpu"):
    """Output storage [rows][width + pad], sentinel-filled."""
    return torch.full((rows, width + pad), SENTINEL, dtype=dtype, device=device)


def window(store, M, width, rmap=None):
    """The [M][width] window of a stored output."""
    return store[row_index(M, rmap, store.device), :width]


def assert_untouched(store, what, rows=None, width=None, region=None):
    """Everything of `store` outside the written window (rows x [0, width), or the boolean mask `region`) still holds the sentinel."""
    masked = store.clone()
    if region is not None:
        masked[region] = SENTINEL
    else:
        masked[rows, :width] = SENTINEL
    assert bool((masked == SENTINEL).all()), f"{what}: {int((masked != SENTINEL).sum())} elements written outside the window"


def strided(x, before, after=8, fill=NAN):
    """x [R][W] as a strided view into a parent [R][before + W + after] whose other columns hold `fill` -> (view, row stride)."""
    R, W = x.shape
    parent = torch.full((R, before + W + after), fill, dtype=x.dtype, device=x.device)
    parent[:, before : before + W] = x
    return parent[:, before:], parent.shape[1]


def rope_tables(rows, half, seed, device="cpu"):
    """f32 [rows][half] cos / sin tables holding bf16-rounded values, positions distinct per row: an input of the launch."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randperm(4096, generator=g)[:rows].float()
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, 2 * half, 2, dtype=F32) / (2 * half)))
    ang = pos[:, None] * inv_freq[None, :]
    return ang.cos().to(BF16).float().to(device), ang.sin().to(BF16).float().to(device)


def rowsq_partials(x, parts, seed):
    """f32 [parts][M]: the rows' sums of squares cut into `parts` uneven non-negative shares (what a producer launch hands over)."""
    g = torch.Generator().manual_seed(seed)
    ss = x.float().pow(2).sum(1).cpu()
    w = torch.rand(parts, x.shape[0], generator=g) + 0.1
    return (w / w.sum(0) * ss).to(F32).to(x.device).contiguous()


def exact_ada_inputs(M, K, B, seed, device="cpu"):
    """x bf16 [M][K], scale / shift f32 [B][K] for which the adaRMS prologue is exact (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor([2.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 0.5])
    vals = base[torch.rand(M, K // 8, 8, generator=g).argsort(-1)]
    sign = torch.randint(0, 2, (M, K // 8, 8), generator=g) * 2.0 - 1.0
    j = torch.randint(-2, 3, (M, 1, 1), generator=g)
    x = (vals * sign * 2.0**j).reshape(M, K).to(BF16)
    scale = torch.randint(-4, 9, (B, K), generator=g).float() / 8.0
    shift = torch.randint(-16, 17, (B, K), generator=g).float() / 16.0
    return x.to(device), scale.to(device), shift.to(device)


def pack_index(N, K):
    """kai0hip.h w_packed, index by index: element offset of W[n][k] = (t * (K / 32) + s) * 512 + (i + 16 g) * 8 + e with n = 16 t + i,
    k = 32 s + 8 g + e -> int64 [N][K]."""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    t, i = n // 16, n % 16
    s, g, e = k // 32, (k % 32) // 8, k % 8
    return (t * (K // 32) + s) * 512 + (i + 16 * g) * 8 + e


# ------------------------------------------------------------------------------------------------ the forms
def product(a, w, dt, ey=None):
    """(acc, err): a [M][K] @ w [N][K]^T in `dt`; err = K * U32 * |A| |W| (+ the operand error e_y of the adaRMS prologue) for the
    f64 reference, None for the emulation."""
    acc = a.to(dt) @ w.to(dt).t()
    if dt != F64:
        return acc, None
    A, W = a.to(F64).abs(), w.to(F64).abs().t()
    if ey is None:
        return acc, a.shape[-1] * U32 * (A @ W)
    return acc, a.shape[-1] * U32 * ((A + ey) @ W) + ey @ W


def partials(a, w, split, dt):
    """split_k > 1: the raw f32 partial products [split][M][N] -> (value, bound or None)."""
    kb = a.shape[-1] // split
    accs, errs = zip(*(product(a[:, s * kb : (s + 1) * kb], w[:, s * kb : (s + 1) * kb], dt) for s in range(split)))
    return torch.stack(accs), None if errs[0] is None else torch.stack(errs) + TINY


def fold(acc, err, rowsq, cvec, K, eps=EPS):
    """The folded adaRMS form on the accumulator: acc * rstd[row] + cvec[n], rstd from the partials as given."""
    parts = rowsq.shape[0]
    if err is None:
        ss = rowsq[0].clone()
        for p in range(1, parts):
            ss = ss + rowsq[p]
        rstd = torch.rsqrt(ss / float(K) + S.f32c(eps))
    else:
        rstd = torch.rsqrt(rowsq.to(F64).sum(0) / K + S.f32c(eps))
    t = acc * rstd[:, None]
    v = t + cvec.to(acc.dtype)[None, :]
    if err is None:
        return v, None
    return v, err * rstd[:, None] + (parts + 4) * U32 * t.abs() + U32 * v.abs()


def linear(acc, err, gate=None, residual=None):
    """Mode 0: bf16 -> * gate -> + residual (gate already expanded to rows).  -> stored bf16, or (ref, bound)."""
    return G.epilogue(acc, err, gate=gate, residual=residual)


def _end(c):
    return c.v.to(BF16) if c.e is None else (c.v, c.e + TINY)


def _sum(a, b):
    c = Chain(a.v, a.e)
    c.f32_op(a.v + b.v, None if a.e is None else a.e + b.e)
    return c


def _times(c, f):
    r = Chain(c.v, c.e)
    r.mul(f)
    r.round_bf16()
    return r


def plain_segment(acc, err):
    c = Chain(acc, err)
    c.round_bf16()
    return _end(c)


def rope(acc, err, cos, sin):
    """acc [M][heads * 2 * half], cos / sin [M][half] (indexed by the A row)."""
    M, W = acc.shape
    half = cos.shape[1]
    x = acc.reshape(M, W // (2 * half), 2, half)
    e = None if err is None else err.reshape(M, W // (2 * half), 2, half)
    c, s = cos.to(acc.dtype)[:, None, :], sin.to(acc.dtype)[:, None, :]
    xs = []
    for i in (0, 1):
        ch = Chain(x[:, :, i], None if e is None else e[:, :, i])
        ch.round_bf16()
        xs.append(ch)
    o1 = _sum(_times(xs[0], c), _times(xs[1], -s))
    o1.round_bf16()
    o2 = _sum(_times(xs[1], c), _times(xs[0], s))
    o2.round_bf16()
    out = Chain(torch.stack([o1.v, o2.v], 2).reshape(M, W), None if err is None else torch.stack([o1.e, o2.e], 2).reshape(M, W))
    return _end(out)


def qkv_segs(H, HD, v_rope=0):
    """(n_begin, n_end, rope) of q | k | v; v plain (0) or stored transposed (2)."""
    return [(0, H * HD, 1), (H * HD, (H + 1) * HD, 1), ((H + 1) * HD, (H + 2) * HD, v_rope)]


def segments(acc, err, segs, cos, sin):
    """Mode 1: one result per column segment, rotated where rope == 1."""
    out = []
    for nb, ne, rp in segs:
        a, e = acc[:, nb:ne], None if err is None else err[:, nb:ne]
        out.append(rope(a, e, cos, sin) if rp == 1 else plain_segment(a, e))
    return out


def gelu_fast(x):
    """common.h gelu_tanh_f in f32: x * (1 - 1 / (exp2(2 u log2 e) + 1)), the exponent's argument as one polynomial times x."""
    beta, kappa, log2e = (torch.tensor(v, dtype=F32) for v in (0.7978845608028654, 0.044715, 1.4426950408889634))
    a0, a1 = 2.0 * beta * log2e, 2.0 * beta * kappa * log2e
    r = 1.0 / (torch.exp2(x * (x * x * a1 + a0)) + 1.0)
    return x * (1.0 - r)


def geglu(acc, err):
    """Mode 2 on acc [M][2 F] = [gate pre-activations | up]."""
    F = acc.shape[1] // 2
    g, u = Chain(acc[:, :F], None if err is None else err[:, :F]), Chain(acc[:, F:], None if err is None else err[:, F:])
    g.round_bf16()
    u.round_bf16()
    if err is None:
        h = Chain(gelu_fast(g.v))
        h.round_bf16()
        h.v = h.v * u.v
        return _end(h)
    c = Chain(Fn.gelu(g.v, approximate="tanh"), L_GELU * g.e + g.v.abs() * (SIG_ERR + 8 * U32))
    c.round_bf16()
    ref = c.v * u.v
    h = Chain(ref, u.v.abs() * c.e + (c.v.abs() + c.e) * u.e + U32 * ref.abs())
    h.round_bf16()
    return _end(h)


def rowsq_out_ref(stored):
    """(ref, bound) f64 [N / 16][M] from the bf16 rows a mode-0 launch stored."""
    x = stored.to(F64)
    M, N = x.shape
    s = (x * x).reshape(M, N // 16, 16).sum(-1).t().contiguous()
    return s, 16 * U32 * s + TINY


def ada_exact(x, scale, shift, rpb, eps=EPS):
    """The exact y of the adaRMS prologue on `exact_ada_inputs` and its operand error e_y (f64 [M][K] both)."""
    X = x.to(F64)
    M = X.shape[0]
    meansq = (X * X).mean(-1, keepdim=True)
    xh = X / meansq.sqrt()
    sc, sh = (t.to(F64).repeat_interleave(rpb, 0)[:M] for t in (scale, shift))
    y = xh * (1 + sc) + sh
    ey = (S.f32c(eps) / (2 * meansq) + 4 * U32) * (xh.abs() * (1 + sc.abs()) + sh.abs())
    return y, torch.where(y != 0, torch.zeros_like(ey), ey)


def ada_emulate(x, scale, shift, rpb, eps=EPS):
    """The f32 prologue with its bf16 rounding (streaming_refs.rmsnorm_fwd is the adaRMS formula), as bf16."""
    return rmsnorm_fwd(x, None, eps, F32, mod=torch.cat([scale, shift], 1), rpb=rpb)["y"].value.to(BF16)
