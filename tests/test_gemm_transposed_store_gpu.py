"""kai0_gemm_bf16's transposed second store (kai0hip.h ct / ct2): the act-0, act-6 and act-3 epilogues of the 256 x 256 NT tile kernel
and of the persistent NT kernel also write what they store row-major as [N][M] matrices.

For each form and each kernel, one launch without and one with the transposed pointers:
  * C, pre_out and pre_out2 are bit-identical between the two launches (the transposed store changes nothing else);
  * CT (and CT2) equal C.t() (pre_out.t()) bit for bit, edge rows and columns of ragged tiles included;
  * the CT buffer lies in a sentinel-filled store — guard rows in front and behind, row padding up to ldct — that must survive;
  * kai0_gemm_plan reports the kernel that runs and the transposed store;
  * every output lies inside a per-element float64 bound: C of act 0 and g, u of act 6 inside tests/gemm_refs.py's own; h of act 6
    and dg, du of act 3 inside the bound that chain carries through the GeGLU arithmetic of kai0hip.h (below).

The GeGLU bounds, derived like gemm_refs.py's and not measured.  (x, e) = (exact f64 value, bound on |computed - exact|):
  linear part    g, u (act 6) and dh (act 3) with their bounds from gemm_refs.reference (accumulation + the bf16 rounding);
  gelu_tanh      exact in f64 on the exact argument.  An argument off by e moves it by at most 1.13 e (|gelu_tanh'| <= 1.129
                 everywhere); its f32 evaluation — a dozen f32 operations, v_exp_f32 and v_rcp_f32 at 1 ulp each, the cancellation
                 in 1 + tanh for negative arguments — is allowed FN = 2^-16 (128 f32 ulps) of |argument|, which bounds |gelu|;
  gelu_tanh'     the same allowance on (1 + |g|)^2, which bounds every term of the derivative's formula;
  f32 multiply   e = |a| eb + |b| ea + ea eb + U32 |a b|;  bf16 rounding  e += UBF (|x| + e)   (gemm_refs.py's two rules);
  act 6          h = bf16(bf16(gelu(g)) * u);   act 3   du = bf16(dh * bf16(gelu(g))),  dg = bf16(bf16(dh * u) * gelu'(g)).

Shapes: the smallest that reach each kernel (>= 160 tiles of 256 x 256 for the tile, >= 512 with persist = 2 for the persistent
kernel): 2560 x 4096 x 256 (full tiles), 2600 x 4104 x 320 (ragged rows and columns), 5120 x 8192 x 256 (persistent) and
5128 x 8200 x 320 (persistent, ragged).  Act 6 needs N % 32 == 0: 4104 -> 4128 and 8200 -> 8224 there, still no multiples of the tile."""

import math

import pytest
import torch

import gemm_refs as R

pytestmark = pytest.mark.gpu

BF16, F64 = torch.bfloat16, torch.float64
GUARD = 3  # sentinel rows in front of and behind CT
CASES = [("tile", 2560, 4096, 256, 1, "quadrant"), ("tile-ragged", 2600, 4104, 320, 1, "quadrant"), ("persistent", 5120, 8192, 256, 2, "persistent"),
         ("persistent-ragged", 5128, 8200, 320, 2, "persistent")]
FN = 2.0**-16  # the f32 evaluation of gelu_tanh / gelu_tanh' (module docstring)
C0, C1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu64(g):
    return 0.5 * g * (1.0 + torch.tanh(C0 * (g + C1 * g**3)))


def dgelu64(g):
    t = torch.tanh(C0 * (g + C1 * g**3))
    return 0.5 * (1.0 + t) + 0.5 * g * (1.0 - t * t) * C0 * (1.0 + 3.0 * C1 * g * g)


def rounded(x, e):
    return e + R.UBF * (x.abs() + e)


def product(a, ea, b, eb):
    p = a * b
    return p, a.abs() * eb + b.abs() * ea + ea * eb + R.U32 * p.abs()


@pytest.fixture(scope="module")
def ops():
    from kai0_amd import ops as _ops

    return _ops


def dev():
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16).to(dev())


def sentinel(*shape):
    return torch.full(shape, R.SENTINEL, dtype=BF16, device=dev())


class CT:
    """[N][M] window with leading dimension M + 16 inside a sentinel-filled store with GUARD rows on either side."""

    def __init__(self, N, M):
        self.N, self.M, self.ld = N, M, M + 16
        self.store = sentinel(N + 2 * GUARD, self.ld)
        self.win = self.store[GUARD : GUARD + N]

    def check(self, c, what):
        torch.cuda.synchronize()
        assert torch.equal(self.win[:, : self.M], c.t()), f"{what}: CT != C.t() ({int((self.win[:, :self.M] != c.t()).sum())} elements differ)"
        masked = self.store.clone()
        masked[GUARD : GUARD + self.N, : self.M] = R.SENTINEL
        assert torch.equal(masked, torch.full_like(masked, R.SENTINEL)), f"{what}: a write outside the [N][M] window of CT"


@pytest.mark.parametrize("name,M,N,K,persist,loop", CASES, ids=[c[0] for c in CASES])
def test_act6_transposed_h(ops, name, M, N, K, persist, loop):
    N = (N + 31) // 32 * 32  # act 6: N % 32 == 0 (4104 -> 4128: still no multiple of the tile)
    x, wg, wu = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((N, K), 3, 0.05)
    outs = []
    with ops.gemm_tuning(persist=persist):
        for with_ct in (False, True):
            h, g, u = sentinel(M, N), sentinel(M, N), sentinel(M, N)
            kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, act=6, B2=wu, pre_out=g, pre_out2=u)
            ct = CT(N, M)
            if with_ct:
                kw.update(ct=ct.win, ldct=ct.ld)
            plan = ops.gemm_plan(x, wg, h, **kw)
            assert (plan["tile"], plan["loop"], plan.get("transposed_store", False)) == (256, loop, with_ct), plan
            ops.gemm(x, wg, h, **kw)
            if with_ct:
                ct.check(h, f"act 6 {name}")
            outs.append((h, g, u))
    torch.cuda.synchronize()
    for a, b, what in zip(outs[0], outs[1], ("h", "g", "u")):
        assert torch.equal(a, b), f"act 6 {name}: {what} differs between the launches with and without the transposed store"
    (g64, eg), (u64, eu) = R.reference(x, wg.t()), R.reference(x, wu.t())
    gl = gelu64(g64)
    h64, eh = product(gl, rounded(gl, 1.13 * eg + FN * (g64.abs() + eg)), u64, eu)
    for got, ref, bound, what in ((outs[1][1], g64, eg, "g"), (outs[1][2], u64, eu, "u"), (outs[1][0], h64, rounded(h64, eh) + R.TINY, "h")):
        print(f"[act 6 {name}] {what}: worst err / bound {R.assert_within(got, ref, bound, what):.3f}")


@pytest.mark.parametrize("name,M,N,K,persist,loop", CASES, ids=[c[0] for c in CASES])
def test_act0_transposed_c(ops, name, M, N, K, persist, loop):
    a, w = rnd((M, K), 8), rnd((N, K), 9, 0.05)
    outs = []
    with ops.gemm_tuning(persist=persist):
        for with_ct in (False, True):
            c = sentinel(M, N)
            kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N)
            ct = CT(N, M)
            if with_ct:
                kw.update(ct=ct.win, ldct=ct.ld)
            plan = ops.gemm_plan(a, w, c, **kw)
            assert (plan["tile"], plan["loop"], plan.get("transposed_store", False)) == (256, loop, with_ct), plan
            ops.gemm(a, w, c, **kw)
            if with_ct:
                ct.check(c, f"act 0 {name}")
            outs.append(c)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), f"act 0 {name}: C differs between the launches with and without the transposed store"
    print(f"[act 0 {name}] C: worst err / bound {R.assert_within(outs[1], *R.reference(a, w.t()), 'C'):.3f}")


@pytest.mark.parametrize("name,M,N,K,persist,loop", CASES, ids=[c[0] for c in CASES])
def test_act3_transposed_dg_du(ops, name, M, N, K, persist, loop):
    dout, wdt, g, u = rnd((M, K), 4), rnd((N, K), 5, 0.05), rnd((M, N), 6), rnd((M, N), 7)
    outs = []
    with ops.gemm_tuning(persist=persist):
        for with_ct in (False, True):
            dg, du = sentinel(M, N), sentinel(M, N)
            kw = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, act=3, pre_out=du, aux1=g, aux2=u)
            ct, ct2 = CT(N, M), CT(N, M)
            if with_ct:
                kw.update(ct=ct.win, ldct=ct.ld, ct2=ct2.win, ldct2=ct2.ld)
            plan = ops.gemm_plan(dout, wdt, dg, **kw)
            assert (plan["tile"], plan["loop"], plan.get("transposed_store", False)) == (256, loop, with_ct), plan
            ops.gemm(dout, wdt, dg, **kw)
            if with_ct:
                ct.check(dg, f"act 3 {name} dg")
                ct2.check(du, f"act 3 {name} du")
            outs.append((dg, du))
    torch.cuda.synchronize()
    for a, b, what in zip(outs[0], outs[1], ("dg", "du")):
        assert torch.equal(a, b), f"act 3 {name}: {what} differs between the launches with and without the transposed store"
        assert not bool((b == R.SENTINEL).any()), f"act 3 {name}: {what} has unwritten elements"
    dh, edh = R.reference(dout, wdt.t())
    g64, u64 = g.to(F64), u.to(F64)
    gl, gr = gelu64(g64), dgelu64(g64)
    du64, edu = product(dh, edh, gl, rounded(gl, FN * g64.abs()))
    t, et = product(dh, edh, u64, 0.0)
    dg64, edg = product(t, rounded(t, et), gr, FN * (1.0 + g64.abs()) ** 2)
    for got, ref, bound, what in ((outs[1][0], dg64, rounded(dg64, edg) + R.TINY, "dg"), (outs[1][1], du64, rounded(du64, edu) + R.TINY, "du")):
        print(f"[act 3 {name}] {what}: worst err / bound {R.assert_within(got, ref, bound, what):.3f}")


def test_transposed_store_is_validated(ops):
    """What the epilogues do not carry is refused, never dropped: split-K, an f32 output, column segments, other acts, act 0 with a
    bias, a problem of the 128 x 128 tile, M % 8 != 0, a short or misaligned ldct, ct2 without ct."""
    from kai0_amd import _lib

    M, N, K = 2560, 4096, 256
    x, w, g, u = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((M, N), 6), rnd((M, N), 7)
    dg, du, ct, ct2 = sentinel(M, N), sentinel(M, N), sentinel(N, M), sentinel(N, M)
    a3 = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N, act=3, pre_out=du, aux1=g, aux2=u, ct=ct, ldct=M, ct2=ct2, ldct2=M)
    ops.gemm_plan(x, w, dg, **a3)  # the base descriptor is valid

    def refused(match, out=dg, **change):
        with pytest.raises(_lib.Kai0HipError, match=match):
            ops.gemm_plan(x, w, out, **{**a3, **change})

    refused("transposed store excludes", split_k=2)
    refused(None, out=torch.empty(M, N, dtype=torch.float32, device=dev()))
    refused(None, segs=[(dg, N, 0)])
    refused("transposed store needs act=0 or act=6 with ct", act=1, pre_out=None, aux1=None, aux2=None, ct2=None)
    refused("transposed store needs act=0 or act=6 with ct", act=0, pre_out=None, aux1=None, aux2=None)
    refused("plain form", act=0, pre_out=None, aux1=None, aux2=None, ct2=None, bias=rnd((N,), 3))
    refused("transposed store needs act=0 or act=6 with ct", ct=None)
    refused("transposed store needs act=0 or act=6 with ct", ct2=None)
    refused("ldct", ldct=M - 8)
    refused("ldct", ldct2=M + 4)
    refused("plain form", residual=dg, ldr=N)
    refused("256 x 256", M=1024)
    refused("M % 8", M=M - 4)
    assert bool((ct == R.SENTINEL).all()) and bool((dg == R.SENTINEL).all())  # (plans launch nothing)
