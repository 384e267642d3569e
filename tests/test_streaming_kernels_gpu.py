"""The streaming kernels (csrc/elementwise.hip, csrc/norm.hip, csrc/optim.hip) past their grid caps and on hard inputs.

Every wrapper caps its grid and the kernel walks the rest of the data in a grid-stride loop; the direct tests of
tests/test_kernels_gpu.py stay below every cap, so each loop makes one trip there.  Here:

  A. one launch past the cap per kernel family (two or more trips and a ragged tail), checked three ways:
       sentinels   every output is pre-filled with NaN and sits between 64 sentinel elements on both sides: no NaN may be left, the
                   sentinels must be untouched;
       slicing     element-wise and row-wise results do not depend on the block that computed them: the one big launch must
                   equal, bit for bit, the same call made over consecutive slices that each fit in one trip;
       reference   per element against the float64 reference of tests/streaming_refs.py.
  B. the register forms, in-place uses, entry points and input distributions nothing else feeds, at small row counts.

Bounds: tests/streaming_refs.py (`ulp |ref| + c sum|terms| + extra`, no outlier share), calibrated without the kernels by
tests/test_streaming_refs_cpu.py.  Every test prints its worst error / bound ratio.  Calls go through the C ABI
(kai0_amd._lib.call) as in tests/test_kernels_gpu.py."""

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streaming_refs as R  # noqa: E402
from streaming_refs import BF16, F32, F64, GUARD, SENTINEL  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
NORM_D = [8, 504, 512, 520, 1024, 1536, 2040, 2048]
SOFTMAX_LD = [512, 520, 1024, 1032, 2048, 2056, 4096]
EPS = 1e-6


def call(name, *args):
    from kai0_amd import _lib

    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def rnd(*shape, dtype=BF16, seed=0, scale=1.0):
    return R.randn(*shape, dtype=dtype, seed=seed, scale=scale, device=DEV)


def P(t):
    return None if t is None else t.data_ptr()


class Out:
    """An output between two bands of GUARD sentinel elements, pre-filled with NaN (or a copy of `init` for in-place kernels).
    `off`: the output starts that many elements past the 16-byte boundary (the front band is that much longer)."""

    def __init__(self, shape, dtype, fill=NAN, init=None, off=0):
        n = math.prod(shape)
        self.front = GUARD + off
        self.buf = torch.full((self.front + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[self.front : self.front + n].view(shape)
        assert self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        if init is not None:
            self.t.copy_(init)
        else:
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.buf[: self.front] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all()), f"{what}: wrote outside its output"
        left = int(torch.isnan(self.t).sum())
        assert left == 0, f"{what}: {left} of {self.t.numel()} elements never written (first at flat index {int(torch.isnan(self.t).reshape(-1).nonzero()[0])})"


def whole_and_sliced(launch, new_outs, total, step, what, not_identical=()):
    """launch(lo, hi, outs) once over [0, total) and again over slices of `step`: sentinels of both, bit-identity of the two."""
    big, small = new_outs(), new_outs()
    launch(0, total, big)
    for lo in range(0, total, step):
        launch(lo, min(total, lo + step), small)
    torch.cuda.synchronize()
    for k in big:
        big[k].check(f"{what}.{k}")
        if k not in not_identical:
            small[k].check(f"{what}.{k} (sliced)")
            same = big[k].t == small[k].t
            assert bool(same.all()), (f"{what}.{k}: one launch differs from the sliced launches in {int((~same).sum())} elements, first at flat index "
                                      f"{int((~same).reshape(-1).nonzero()[0])} of {same.numel()}")
    return big


RATIOS = {}


def within(out, res, what, c=R.C0):
    r = R.assert_within(out, res, what, c=c)
    RATIOS[what] = r
    print(f"worst error/bound {what}: {r:.3f}")
    return r


def exact(out, want, what):
    same = out == want
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ from the single-rounding result, first at {int((~same).reshape(-1).nonzero()[0])}"


# =================================================================================================== A. norms
def _norm_params(kind, D, B=0):
    if kind == "rms":
        return dict(w=rnd(D, dtype=F32, seed=5, scale=0.3))
    if kind == "ada":
        return dict(mod=rnd(B, 3 * D, dtype=F32, seed=6, scale=0.3))
    return dict(w=(1 + rnd(D, seed=5, scale=0.2).float()).to(BF16), b=rnd(D, seed=6, scale=0.2))


def _norm_fwd_launch(kind, x, p, rpb, D):
    def launch(lo, hi, o):
        n = hi - lo
        if kind == "rms":
            call("kai0_rmsnorm_fwd", P(x[lo:]), P(p["w"]), P(o["y"].t[lo:]), P(o["rstd"].t[lo:]), n, D, EPS)
        elif kind == "ada":
            b0 = lo // rpb
            call("kai0_adarms_fwd", P(x[lo:]), P(p["mod"][b0:]), P(o["y"].t[lo:]), P(o["gate"].t[b0:]), P(o["rstd"].t[lo:]), n, rpb, D, EPS)
        else:
            call("kai0_layernorm_fwd", P(x[lo:]), P(p["w"]), P(p["b"]), P(o["y"].t[lo:]), P(o["mean"].t[lo:]), P(o["rstd"].t[lo:]), n, D, EPS)
    return launch


def _norm_fwd_outs(kind, rows, D, B):
    def new():
        o = dict(y=Out((rows, D), BF16), rstd=Out((rows,), F32))
        if kind == "ada":
            o["gate"] = Out((B, D), BF16)
        if kind == "ln":
            o["mean"] = Out((rows,), F32)
        return o
    return new


def _norm_fwd_check(kind, o, x, p, rpb, D, what):
    if kind == "ln":
        ref = R.layernorm_fwd(x, p["w"], p["b"], EPS, F64)
        within(o["mean"].t, ref["mean"], f"{what}.mean")
    else:
        ref = R.rmsnorm_fwd(x, p.get("w"), EPS, F64, mod=p.get("mod"), rpb=rpb)
    within(o["y"].t, ref["y"], f"{what}.y")
    within(o["rstd"].t, ref["rstd"], f"{what}.rstd")
    if kind == "ada":
        exact(o["gate"].t, p["mod"][:, 2 * D :].to(BF16), f"{what}.gate")


@pytest.mark.parametrize("D", [64, 1152])
@pytest.mark.parametrize("kind", ["rms", "ada", "ln"])
def test_norm_fwd_past_the_grid_cap(kind, D):
    """norm_grid: 2048 blocks x 4 waves = 8192 rows a trip; 2 * 8192 + 5 rows = two trips and five rows (D = 1152: a partial
    third chunk of 8 columns per lane).  adaRMS: 37 rows per batch entry, the last entry cut short."""
    rows, rpb = 2 * 8192 + 5, 37
    B = -(-rows // rpb)
    x, p = rnd(rows, D, seed=1), _norm_params(kind, D, B)
    o = whole_and_sliced(_norm_fwd_launch(kind, x, p, rpb, D), _norm_fwd_outs(kind, rows, D, B), rows, 37 * 221, f"{kind}_fwd D={D}")
    _norm_fwd_check(kind, o, x, p, rpb, D, f"A {kind}_fwd D={D}")


def _norm_stats(kind, x, p, rpb, D):
    rows = x.shape[0]
    o = _norm_fwd_outs(kind, rows, D, rows // rpb if kind == "ada" else 0)()
    _norm_fwd_launch(kind, x, p, rpb, D)(0, rows, o)
    return o


def _norm_bwd(kind, x, dy, dres, dgate, p, st, rpb, D, step, what):
    """dx (+ dmod) under slicing; the column sums (dw | db through kai0_reduce_partials, dmod) against the reference."""
    from kai0_amd.ops import NORM_PARTIAL_BLOCKS as NB

    rows = x.shape[0]
    rstd = st["rstd"].t
    W = {"rms": D, "ln": 2 * D}.get(kind)

    def new():
        o = dict(dx=Out((rows, D), BF16))
        if kind == "ada":
            o["dmod"] = Out((rows // rpb, 3 * D), F32)
        else:
            o["part"] = Out((NB, W), F32)
        return o

    def launch(lo, hi, o):
        n = hi - lo
        dr = P(dres[lo:]) if dres is not None else None
        if kind == "rms":
            call("kai0_rmsnorm_bwd", P(dy[lo:]), P(x[lo:]), P(p["w"]), P(rstd[lo:]), P(o["dx"].t[lo:]), P(o["part"].t), NB, dr, n, D)
        elif kind == "ln":
            call("kai0_layernorm_bwd", P(dy[lo:]), P(x[lo:]), P(p["w"]), P(st["mean"].t[lo:]), P(rstd[lo:]), P(o["dx"].t[lo:]), P(o["part"].t), NB,
                 dr, n, D)
        else:
            b0 = lo // rpb
            call("kai0_adarms_bwd", P(dy[lo:]), P(dgate[b0:]) if dgate is not None else None, P(x[lo:]), P(p["mod"][b0:]), P(rstd[lo:]),
                 P(o["dx"].t[lo:]), P(o["dmod"].t[b0:]), dr, n, rpb, D)

    o = whole_and_sliced(launch, new, rows, step, what, not_identical=("part",))
    if kind == "ln":
        ref = R.layernorm_bwd(dy, x, p["w"], st["mean"].t, rstd, dres, F64)
        dw, db = Out((D,), BF16), Out((D,), BF16)
        call("kai0_reduce_partials", P(o["part"].t), NB, D, 2 * D, P(dw.t), 0)
        call("kai0_reduce_partials", o["part"].t.data_ptr() + 4 * D, NB, D, 2 * D, P(db.t), 0)
        for nm, t in (("dw", dw), ("db", db)):
            t.check(f"{what}.{nm}")
            within(t.t, ref[nm], f"{what}.{nm}")
    else:
        ref = R.rmsnorm_bwd(dy, x, p.get("w"), rstd, dres, F64, mod=p.get("mod"), rpb=rpb, dgate=dgate)
        if kind == "rms":
            dw = Out((D,), F32)
            call("kai0_reduce_partials", P(o["part"].t), NB, D, D, P(dw.t), 1)
            dw.check(f"{what}.dw")
            within(dw.t, ref["dw"], f"{what}.dw")
        else:
            within(o["dmod"].t, ref["dmod"], f"{what}.dmod")
            gd = o["dmod"].t[:, 2 * D :]
            exact(gd, dgate.float() if dgate is not None else torch.zeros_like(gd), f"{what}.dgate passthrough")
    within(o["dx"].t, ref["dx"], f"{what}.dx")


@pytest.mark.parametrize("D", [64, 1152])
@pytest.mark.parametrize("kind", ["rms", "ln"])
def test_norm_bwd_past_the_partial_blocks(kind, D):
    """NORM_PARTIAL_BLOCKS = 512 blocks x 4 waves = 2048 rows a trip: at 3 * 2048 + 3 rows a wave accumulates its dw (| db)
    registers over three trips and three waves over a fourth."""
    rows = 3 * 2048 + 3
    x, dy, dres = rnd(rows, D, seed=1), rnd(rows, D, seed=2), rnd(rows, D, seed=3)
    p = _norm_params(kind, D)
    st = _norm_stats(kind, x, p, 1, D)
    _norm_bwd(kind, x, dy, dres, None, p, st, 1, D, 2048, f"A {kind}_bwd D={D}")


@pytest.mark.parametrize("D", [64, 1152])
def test_adarms_bwd_rows_not_a_multiple_of_its_waves(D):
    """One block of 8 waves per batch entry walks rpb = 21 rows (i += 8): two full trips and five waves on a third."""
    B, rpb = 3, 21
    x, dy, dres, dgate = rnd(B * rpb, D, seed=1), rnd(B * rpb, D, seed=2), rnd(B * rpb, D, seed=3), rnd(B, D, seed=4)
    p = _norm_params("ada", D, B)
    st = _norm_stats("ada", x, p, rpb, D)
    _norm_bwd("ada", x, dy, dres, dgate, p, st, rpb, D, rpb, f"A ada_bwd D={D}")


# =================================================================================================== B. norms on hard rows
@pytest.mark.parametrize("D", NORM_D)
@pytest.mark.parametrize("kind", ["rms", "ada", "ln"])
def test_norm_fwd_bwd_on_hard_rows(kind, D):
    """Zero rows, constant rows (a one-pass variance would go negative inside rsqrt), a constant row with one element one bf16 ulp
    up, 100 + N(0,1), 1e4 N(0,1), 1e-4 N(0,1), N(0,1) — at every chunk boundary of the 8-columns-per-lane layout, and at D = 2048
    where the backward kernels' dynamic LDS is at its largest (LayerNorm: 8 D floats = exactly 64 KiB)."""
    rpb, B = 7, 3
    x = R.hard_rows(B, D, seed=D).to(DEV)
    rows = x.shape[0]
    dy, dres, dgate = rnd(rows, D, seed=2), rnd(rows, D, seed=3), rnd(B, D, seed=4)
    p = _norm_params(kind, D, B)
    st = _norm_stats(kind, x, p, rpb, D)
    for k in st:
        st[k].check(f"{kind}_fwd.{k}")
    what = f"B {kind} D={D}"
    _norm_fwd_check(kind, st, x, p, rpb, D, what + " fwd")
    if kind == "rms":
        assert float(st["y"].t[0::7].float().abs().max()) == 0.0  # zero rows stay zero
    step = rpb if kind == "ada" else rows
    for dr in (dres, None):
        for dg in ((dgate, None) if kind == "ada" else (None,)):
            _norm_bwd(kind, x, dy, dr, dg, p, st, rpb, D, step, f"{what} bwd dres={dr is not None}" + (f" dgate={dg is not None}" if kind == "ada" else ""))


# =================================================================================================== softmax
def _softmax_fwd(scores, probs, qcode, kcode, B, Sq, H, Sk, ld, q0):
    call("kai0_softmax_mask_fwd", P(scores), P(probs), P(qcode), P(kcode), B, Sq, H, Sk, ld, Sq * H * ld, q0,
         qcode.stride(0) if qcode is not None else 0, kcode.stride(0) if kcode is not None else 0)


def test_softmax_fwd_bwd_past_the_grid_cap():
    """ew_grid(rows, 4): 8192 blocks x 4 rows = 32 768 rows a trip; B = 2, Sq = 24, H = 700 is 33 600 rows: the second trip starts
    inside batch entry 1.  Prefix-LM mask, q0 = Sk - Sq, Sk = 43 in ld = 48 (Sk % 8 != 0: the clamped scalar key-code path)."""
    B, Sq, H, Sk, ld = 2, 24, 700, 43, 48
    M, q0 = Sq * H, Sk - Sq
    scores = rnd(B, M, ld, seed=1, scale=3.0)
    pad = torch.ones(B, Sk, dtype=torch.bool, device=DEV)
    pad[0, 10:14] = False
    pad[1, 30:] = False
    pad[1, 2] = False
    att = torch.zeros(B, Sk, dtype=torch.bool, device=DEV)
    att[:, 35] = True
    qcode, kcode = R.codes_from_pad_att(pad, att)

    def launch(lo, hi, o):  # lo, hi: batch entries
        _softmax_fwd(scores[lo:], o["probs"].t[lo:], qcode[lo:], kcode[lo:], hi - lo, Sq, H, Sk, ld, q0)

    o = whole_and_sliced(launch, lambda: dict(probs=Out((B, M, ld), BF16)), B, 1, "A softmax_fwd")
    allowed = R.allowed_mask(qcode, kcode, Sq, Sk, q0).repeat_interleave(H, 1)
    within(o["probs"].t, R.softmax_fwd(scores, allowed, Sk, F64)["probs"], "A softmax_fwd.probs")
    probs = o["probs"].t.reshape(B * M, ld)
    assert float(probs.view(B, Sq, H, ld)[1, 30 - q0 :].float().abs().max()) == 0.0  # padded queries: zeros
    for f32 in (0, 1):
        dp = rnd(B * M, ld, dtype=F32 if f32 else BF16, seed=2)

        def launch_b(lo, hi, o):
            call("kai0_softmax_bwd", P(probs[lo:]), P(dp[lo:]), f32, P(o["ds"].t[lo:]), hi - lo, Sk, ld, 0.5)

        ob = whole_and_sliced(launch_b, lambda: dict(ds=Out((B * M, ld), BF16)), B * M, 16800, f"A softmax_bwd f32={f32}")
        within(ob["ds"].t, R.softmax_bwd(probs, dp, Sk, 0.5, F64)["dscores"], f"A softmax_bwd f32={f32}")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ld", SOFTMAX_LD)
def test_softmax_fwd_register_forms_and_edge_rows(ld, masked):
    """The four register forms (ld <= 512 / 1024 / 2048 / 4096) and the first width past each; Sk = ld - 5, 2 x 37 rows.  Rows:
    all-equal logits, equal logits of 3e4, a spread of +-80, N(0,1) x 3; masked: queries that see nothing (zeros) and queries
    that see exactly one key (exactly 1.0 there); the key codes with an ODD leading dimension, so batch entry 1's code row is not
    16-byte aligned and takes the scalar path.  In place (probs == scores) is bit-identical to out of place."""
    rows, Sk = 37, ld - 5
    q0 = Sk - rows
    scores, qcode, kcode, allowed = R.softmax_case(ld, masked, seed=ld, device=DEV)
    if masked:
        assert Sk % 2 == 1
        assert kcode.stride(0) % 4 != 0  # odd leading dimension: entry 1 is 4-byte but not 16-byte aligned
    out = Out((2, rows, ld), BF16)
    _softmax_fwd(scores, out.t, qcode, kcode, 2, rows, 1, Sk, ld, q0)
    out.check("softmax_fwd")
    within(out.t, R.softmax_fwd(scores, allowed, Sk, F64)["probs"], f"B softmax_fwd ld={ld} masked={masked}")
    assert float(out.t[..., Sk:].float().abs().max()) == 0.0
    if masked:
        assert float(out.t[:, [4, 9]].float().abs().max()) == 0.0
        one = out.t[:, [6, 11]].float()
        assert bool((one[..., Sk - 3] == 1.0).all()) and float(one.sum()) == 4.0
    inplace = Out((2, rows, ld), BF16, init=scores)
    _softmax_fwd(inplace.t, inplace.t, qcode, kcode, 2, rows, 1, Sk, ld, q0)
    inplace.check("softmax_fwd in place")
    exact(inplace.t, out.t, "softmax_fwd in place")


@pytest.mark.parametrize("ld", SOFTMAX_LD)
def test_softmax_bwd_on_uniform_rows(ld):
    """Near-uniform attention: dprobs - <dprobs, probs> cancels (kai0hip.h); bf16 and f32 dprobs, every width of the forward's list."""
    rows, Sk = 37, ld - 5
    probs = torch.full((rows, ld), 1.0 / Sk, device=DEV).to(BF16)
    probs[:, Sk:] = 3.0  # the padding columns must read as zero
    for f32 in (0, 1):
        dp = rnd(rows, ld, dtype=F32 if f32 else BF16, seed=3 + f32)
        ds = Out((rows, ld), BF16)
        call("kai0_softmax_bwd", P(probs), P(dp), f32, P(ds.t), rows, Sk, ld, 0.5)
        ds.check("softmax_bwd")
        within(ds.t, R.softmax_bwd(probs, dp, Sk, 0.5, F64)["dscores"], f"B softmax_bwd ld={ld} f32={f32}")
        assert float(ds.t[:, Sk:].float().abs().max()) == 0.0


# =================================================================================================== rowdot, RoPE
@pytest.mark.parametrize("rows,D,step", [(65536 + 9, 256, 32768), (4099, 8, 1024), (4099, 72, 1000), (4099, 512, 1000)])
def test_rowdot_past_the_grid_cap_and_lane_spans(rows, D, step):
    """8192 blocks x 4 waves x (64 / span) rows: 65 536 rows a trip at D = 256; D = 72 reserves 16 lanes for 9, D = 8 packs 64
    rows into a wave, D = 512 is one row per wave."""
    a, b = rnd(rows, D, seed=1), rnd(rows, D, seed=2)

    def launch(lo, hi, o):
        call("kai0_rowdot_bf16", P(a[lo:]), P(b[lo:]), P(o["out"].t[lo:]), hi - lo, D)

    o = whole_and_sliced(launch, lambda: dict(out=Out((rows,), F32)), rows, step, f"rowdot D={D}")
    within(o["out"].t, R.rowdot(a, b, F64)["out"], f"A rowdot rows={rows} D={D}")


def _rope_inputs():
    B, S, HD = 2, 32805, 256
    x = rnd(B, S, HD, seed=1)
    pos = torch.randint(0, 1100, (B, S), device=DEV, dtype=torch.int32, generator=torch.Generator(device=DEV).manual_seed(2))
    inv = (1.0 / (10000.0 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))).to(DEV)
    return B, S, HD, x, pos, inv


@pytest.mark.parametrize("inverse", [0, 1])
def test_rope_inplace_past_the_grid_cap(inverse):
    """8192 blocks x 256 / (HD / 8) = 8 rows: 65 536 rows a trip at HD = 256; B = 2, S = 32 805 is 65 610.  The criteria of
    test_rope (two libms), the slicing identity (one launch per batch entry) and the sentinels."""
    B, S, HD, x, pos, inv = _rope_inputs()

    def launch(lo, hi, o):
        call("kai0_rope_inplace", P(o["x"].t[lo:]), P(pos[lo:]), P(inv), hi - lo, S, S, 0, 1, HD, inverse)

    o = whole_and_sliced(launch, lambda: dict(x=Out((B, S, HD), BF16, init=x)), B, 1, "rope_inplace")
    mism, rel = R.rope_close(o["x"].t.view(B, S, 1, HD), R.rope_ref(x.view(B, S, 1, HD), pos, inv, bool(inverse)))
    print(f"rope_inplace inverse={inverse}: mismatch share {mism:.2e}, rel-L2 {rel:.2e}")
    assert mism < 2e-2 and rel < 3e-3, f"mismatch share {mism:.3e}, rel-L2 {rel:.3e}"


def test_rope_copy_past_the_grid_cap():
    """kai0_rope_copy, strided: source rows of 264 elements, destination rows of 272; sliced along S (16 384 positions x 2)."""
    B, S, HD, x, pos, inv = _rope_inputs()
    sld, dld = HD + 8, HD + 16
    src = torch.full((B, S, sld), 5.0, dtype=BF16, device=DEV)
    src[..., :HD] = x

    def launch(lo, hi, o):
        call("kai0_rope_copy", P(src[:, lo:]), P(o["y"].t[:, lo:]), P(pos[:, lo:]), P(inv), B, hi - lo, 1, HD, S * sld, sld, S * dld, dld, S, 0)

    def new():
        o = dict(y=Out((B, S, dld), BF16))
        o["y"].t[..., HD:] = 9.0  # the gap between destination rows must stay
        return o

    o = whole_and_sliced(launch, new, S, 16384, "rope_copy")
    assert bool((o["y"].t[..., HD:] == 9.0).all())
    mism, rel = R.rope_close(o["y"].t[..., :HD].reshape(B, S, 1, HD), R.rope_ref(x.view(B, S, 1, HD), pos, inv))
    print(f"rope_copy: mismatch share {mism:.2e}, rel-L2 {rel:.2e}")
    assert mism < 2e-2 and rel < 3e-3, f"mismatch share {mism:.3e}, rel-L2 {rel:.3e}"


# =================================================================================================== bf16 element-wise
N16 = 2**24 + 8 * 37  # ew_grid(n / 8, 256): 8192 blocks x 256 lanes x 8 elements = 2^24 a trip
STEP16 = 2**23


def _saturated_exact(out, ref, pre, what):
    sat = R.gelu_saturated(pre)
    exact(out[sat], ref.value[sat].to(out.dtype), f"{what} where the sigmoid saturates")


def test_geglu_fwd_past_the_grid_cap_and_in_place():
    g = R.mix_gelu_points(rnd(N16, seed=1, scale=3.0))
    u = rnd(N16, seed=2)

    def launch(lo, hi, o):
        call("kai0_geglu_fwd", P(g[lo:]), P(u[lo:]), P(o["h"].t[lo:]), hi - lo)

    o = whole_and_sliced(launch, lambda: dict(h=Out((N16,), BF16)), N16, STEP16, "geglu_fwd")
    ref = R.geglu_fwd(g, u, F64)["h"]
    within(o["h"].t, ref, "A geglu_fwd")
    _saturated_exact(o["h"].t, ref, g, "geglu_fwd")
    inplace = Out((N16,), BF16, init=g)  # infer.py: h == g
    call("kai0_geglu_fwd", P(inplace.t), P(u), P(inplace.t), N16)
    inplace.check("geglu_fwd in place")
    exact(inplace.t, o["h"].t, "geglu_fwd in place")


def test_geglu_bwd_past_the_grid_cap():
    g = R.mix_gelu_points(rnd(N16, seed=1, scale=3.0))
    u, dh = rnd(N16, seed=2), rnd(N16, seed=3)

    def launch(lo, hi, o):
        call("kai0_geglu_bwd", P(dh[lo:]), P(g[lo:]), P(u[lo:]), P(o["dg"].t[lo:]), P(o["du"].t[lo:]), hi - lo)

    o = whole_and_sliced(launch, lambda: dict(dg=Out((N16,), BF16), du=Out((N16,), BF16)), N16, STEP16, "geglu_bwd")
    ref = R.geglu_bwd(dh, g, u, F64)
    for k in ("dg", "du"):
        within(o[k].t, ref[k], f"A geglu_bwd.{k}")
        _saturated_exact(o[k].t, ref[k], g, f"geglu_bwd.{k}")


def test_gelu_bwd_past_the_grid_cap():
    pre = R.mix_gelu_points(rnd(N16, seed=1, scale=3.0))
    dy = rnd(N16, seed=2)

    def launch(lo, hi, o):
        call("kai0_gelu_bwd", P(dy[lo:]), P(pre[lo:]), P(o["dx"].t[lo:]), hi - lo)

    o = whole_and_sliced(launch, lambda: dict(dx=Out((N16,), BF16)), N16, STEP16, "gelu_bwd")
    ref = R.gelu_bwd(dy, pre, F64)["dx"]
    within(o["dx"].t, ref, "A gelu_bwd")
    _saturated_exact(o["dx"].t, ref, pre, "gelu_bwd")


def test_gelu_family_on_the_tails():
    """A deterministic grid over [-12, 12] and {+-0, +-30, +-100, +-1e4} as pre-activations, N(0,1) for the other operands: the
    three element-wise kernels, and the GEMM epilogue (act = 1) on one 128 x 128 tile through an identity weight."""
    from kai0_amd import ops

    n = 128 * 128
    pre, a, b = R.gelu_points(n, DEV), rnd(n, seed=1), rnd(n, seed=2)
    h, dg, du, dx = (Out((n,), BF16) for _ in range(4))
    call("kai0_geglu_fwd", P(pre), P(a), P(h.t), n)
    call("kai0_geglu_bwd", P(b), P(pre), P(a), P(dg.t), P(du.t), n)
    call("kai0_gelu_bwd", P(a), P(pre), P(dx.t), n)
    rb_ = R.geglu_bwd(b, pre, a, F64)
    for nm, o, ref in (("geglu_fwd", h, R.geglu_fwd(pre, a, F64)["h"]), ("geglu_bwd.dg", dg, rb_["dg"]), ("geglu_bwd.du", du, rb_["du"]),
                       ("gelu_bwd", dx, R.gelu_bwd(a, pre, F64)["dx"])):
        o.check(nm)
        within(o.t, ref, f"B {nm} tails")
        _saturated_exact(o.t, ref, pre, nm)
    y = ops.linear_fwd(pre.view(128, 128), torch.eye(128, dtype=BF16, device=DEV), act=1)
    ref = R.gelu_fwd(pre, F64)["y"]
    within(y.reshape(-1), ref, "B linear act=1 tails")
    _saturated_exact(y.reshape(-1), ref, pre, "linear act=1")


@pytest.mark.parametrize("tail", [0, 5])
def test_casts_and_add_bf16_past_the_grid_cap(tail):
    """n = 2^24 + 8 * 37 (+ 5: the scalar tail that block 0 handles after its vector loop)."""
    n = N16 + tail
    x, a, b = rnd(n, dtype=F32, seed=1), rnd(n, seed=2), rnd(n, seed=3)

    def launch(lo, hi, o):
        call("kai0_cast_f32_to_bf16", P(x[lo:]), P(o["f2b"].t[lo:]), hi - lo)
        call("kai0_cast_bf16_to_f32", P(a[lo:]), P(o["b2f"].t[lo:]), hi - lo)
        call("kai0_add_bf16", P(a[lo:]), P(b[lo:]), P(o["add"].t[lo:]), hi - lo)

    o = whole_and_sliced(launch, lambda: dict(f2b=Out((n,), BF16), b2f=Out((n,), F32), add=Out((n,), BF16)), n, STEP16, f"casts tail={tail}")
    exact(o["f2b"].t, x.to(BF16), "cast_f32_to_bf16")
    exact(o["b2f"].t, a.float(), "cast_bf16_to_f32")
    exact(o["add"].t, (a.float() + b.float()).to(BF16), "add_bf16")


def test_gated_fwd_past_the_grid_cap():
    """rows x D / 8 = 2^21 + 37 items of 8 columns; three batch entries of 699 063 rows."""
    D, rpb, B = 8, 699063, 3
    rows = B * rpb
    assert rows * D == N16
    x, y, gate = rnd(rows, D, seed=1), rnd(rows, D, seed=2), rnd(B, D, seed=3)

    def launch(lo, hi, o):
        call("kai0_gated_fwd", P(x[lo:]), P(y[lo:]), P(gate[lo // rpb :]), P(o["out"].t[lo:]), hi - lo, rpb, D)

    o = whole_and_sliced(launch, lambda: dict(out=Out((rows, D), BF16)), rows, rpb, "gated_fwd")
    exact(o["out"].t, R.gated_fwd_exact(x, y, gate, rpb), "gated_fwd")


# =================================================================================================== f32 element-wise
N32 = 2**21 + 77  # ew_grid(n, 256): 8192 blocks x 256 lanes = 2^21 a trip
STEP32 = 2**20


def test_silu_mse_euler_add_f32_past_the_grid_cap():
    n = N32
    x = R.mix_gelu_points(rnd(n, seed=1, scale=3.0)).float() * 1.0009765625
    a, b, c3 = (rnd(n, dtype=F32, seed=s) for s in (2, 3, 4))

    def launch(lo, hi, o):
        m = hi - lo
        call("kai0_silu_fwd_f32", P(x[lo:]), P(o["silu"].t[lo:]), m)
        call("kai0_silu_bwd_f32", P(a[lo:]), P(x[lo:]), P(o["dsilu"].t[lo:]), m)
        call("kai0_mse_fwd", P(a[lo:]), P(b[lo:]), P(o["loss"].t[lo:]), m)
        call("kai0_mse_bwd", P(a[lo:]), P(b[lo:]), P(c3[lo:]), P(o["dv"].t[lo:]), m)
        call("kai0_euler_step", P(o["euler"].t[lo:]), P(b[lo:]), -0.1, m)
        call("kai0_add_f32", P(a[lo:]), P(b[lo:]), P(o["add"].t[lo:]), m)

    def new():
        o = {k: Out((n,), F32) for k in ("silu", "dsilu", "loss", "dv", "add")}
        o["euler"] = Out((n,), F32, init=a)
        return o

    o = whole_and_sliced(launch, new, n, STEP32, "f32 element-wise")
    within(o["silu"].t, R.silu_fwd(x, F64)["y"], "A silu_fwd")
    within(o["dsilu"].t, R.silu_bwd(a, x, F64)["dx"], "A silu_bwd")
    within(o["loss"].t, R.mse_fwd(a, b, F64)["loss"], "A mse_fwd")
    within(o["dv"].t, R.mse_bwd(a, b, c3, F64)["dv"], "A mse_bwd")
    within(o["euler"].t, R.euler(a, b, -0.1, F64)["x"], "A euler_step")
    exact(o["add"].t, a + b, "add_f32")


def test_flow_mix_add_pos_cast_im2col_past_the_grid_cap():
    B, HA = 13, 161326  # 2 097 238 elements
    nz, ac = rnd(B, HA, dtype=F32, seed=1), rnd(B, HA, dtype=F32, seed=2)
    t = (torch.rand(B, generator=torch.Generator().manual_seed(0)) * 0.999 + 0.001).to(DEV)

    def launch(lo, hi, o):
        call("kai0_flow_mix", P(nz[lo:]), P(ac[lo:]), P(t[lo:]), P(o["xt"].t[lo:]), P(o["ut"].t[lo:]), hi - lo, HA)

    o = whole_and_sliced(launch, lambda: dict(xt=Out((B, HA), F32), ut=Out((B, HA), F32)), B, 6, "flow_mix")
    ref = R.flow_mix(nz, ac, t, F64)
    within(o["xt"].t, ref["xt"], "A flow_mix.xt")
    within(o["ut"].t, ref["ut"], "A flow_mix.ut")

    rows, D, n_pos = 27237, 77, 100  # 2 097 249 elements
    x, pos = rnd(rows, D, dtype=F32, seed=3), rnd(n_pos, D, dtype=F32, seed=4)

    def launch2(lo, hi, o):
        call("kai0_add_pos_cast", P(x[lo:]), P(pos), P(o["out"].t[lo:]), hi - lo, n_pos, D)

    o = whole_and_sliced(launch2, lambda: dict(out=Out((rows, D), BF16)), rows, 13600, "add_pos_cast")
    exact(o["out"].t, (x + pos[torch.arange(rows, device=DEV) % n_pos]).to(BF16), "add_pos_cast")

    n_img, HW, Pp = 223, 56, 14  # 223 x 16 patches x 588 = 2 097 984 elements
    img = rnd(n_img, 3, HW, HW, dtype=F32, seed=5)
    per = (HW // Pp) ** 2

    def launch3(lo, hi, o):
        call("kai0_patch_im2col", P(img[lo:]), P(o["cols"].t[lo * per :]), hi - lo, 3, HW, Pp)

    o = whole_and_sliced(launch3, lambda: dict(cols=Out((n_img * per, 3 * Pp * Pp), F32)), n_img, 111, "im2col")
    exact(o["cols"].t, R.im2col_ref(img, Pp), "patch_im2col")


# =================================================================================================== reductions, optimizer
@pytest.mark.parametrize("is_f32,n", [(0, 2**23 + 8 * 333 + 5), (1, 2**22 + 4 * 333 + 3)])
def test_sumsq_past_the_grid_cap(is_f32, n):
    """opt_grid: 4096 blocks x 256 lanes = 2^20 vectors a trip (8 bf16 / 4 f32 elements each): one full trip, 333 vectors of a second
    and a scalar tail.  All addends are non-negative: the bound is the chain length of f32 additions (streaming_refs.sumsq_chain)
    x 2^-24, relative."""
    g = rnd(n, dtype=F32 if is_f32 else BF16, seed=1)
    out, scratch = Out((1,), F32, fill=0.0), Out((4096,), F32)
    call("kai0_sumsq", P(g), is_f32, n, P(out.t), P(scratch.t))
    torch.cuda.synchronize()
    out.check("sumsq.out")
    scratch.check("sumsq.scratch")
    ref = float(R.sumsq(g, F64))
    L = R.sumsq_chain(n, bool(is_f32))
    bnd = (2.0**-23 + L * 2.0**-24) * ref
    r = abs(float(out.t[0]) - ref) / bnd
    print(f"worst error/bound A sumsq f32={is_f32}: {r:.3f} (chain {L})")
    assert r <= 1.0, f"sumsq: {float(out.t[0])!r} vs {ref!r}: error/bound {r:.3f}"
    again = Out((1,), F32, fill=0.0)  # accumulates into out[0]; reproducible bit for bit
    call("kai0_sumsq", P(g), is_f32, n, P(again.t), P(scratch.t))
    call("kai0_sumsq", P(g), is_f32, n, P(again.t), P(scratch.t))
    assert float(again.t[0]) == float(out.t[0] + out.t[0])


def test_sum_chunks_past_the_grid_cap():
    n = 8 * (2**20 + 5)
    src = rnd(2, n, seed=1)

    def launch(lo, hi, o):
        call("kai0_sum_chunks", P(src[0, lo:]), 0, 2, n, hi - lo, P(o["dst"].t[lo:]))

    o = whole_and_sliced(launch, lambda: dict(dst=Out((n,), BF16)), n, 8 * 2**19, "sum_chunks")
    exact(o["dst"].t, (src[0].float() + src[1].float()).to(BF16), "sum_chunks")


ADAM = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=1e-2, bc1=1 - 0.9**3, bc2=1 - 0.95**3)


def _adam_args(k):
    return k["lr"], k["b1"], k["b2"], k["eps"], k["wd"], k["bc1"], k["bc2"]


def test_adamw_past_the_grid_cap():
    """n = 2^20 + 4099, bf16 gradient and model copy, clip coefficient from device memory.  With every stream 16-byte aligned the
    vectors go one per lane (one contiguous run of 256 per block, 1025 blocks + 3 tail elements): no cap is passed — the vector
    path caps its grid at 2^22 blocks, i.e. past 2^32 elements, which no test reaches (for the EMA form neither);
    kai0_grad_accum with its 4096-block cap walks the same per-block run loop (tests/test_grad_accum_gpu.py).  With the f32
    streams one element in and the 16-bit ones aligned there is no common head: the scalar form, grid-strided over opt_grid's
    4096 blocks x 256 lanes = 2^20 elements a trip, takes a second trip."""
    n = 2**20 + 4099
    master0 = rnd(n, seed=1, scale=0.02).float()
    m0, v0 = rnd(n, dtype=F32, seed=2, scale=1e-2), rnd(n, dtype=F32, seed=3, scale=1e-2).abs()
    grad, coef = rnd(n, seed=4), torch.tensor([0.37], device=DEV)
    ref = R.adamw(master0, m0, v0, grad, coef, *_adam_args(ADAM), F64)

    def launch(lo, hi, o):
        call("kai0_adamw", P(o["master"].t[lo:]), P(o["m"].t[lo:]), P(o["v"].t[lo:]), P(grad[lo:]), 0, P(o["param"].t[lo:]), 0, hi - lo,
             *_adam_args(ADAM), P(coef))

    for what, off32 in (("adamw", 0), ("adamw no common head", 1)):

        def new():
            return dict(master=Out((n,), F32, init=master0, off=off32), m=Out((n,), F32, init=m0, off=off32),
                        v=Out((n,), F32, init=v0, off=off32), param=Out((n,), BF16))  # fmt: skip

        o = whole_and_sliced(launch, new, n, 2**19, what)
        for k in ("master", "m", "v"):
            within(o[k].t, ref[k], f"A {what}.{k}")
        exact(o["param"].t, o["master"].t.to(BF16), f"{what} model copy")


ADAMW_N = (1, 3, 5, 255, 1027, 4099)
# elements past a 16-byte boundary at which the f32 / the 16-bit streams start
ADAMW_LAYOUTS = {"aligned": (0, 0), "one_in": (1, 1), "no_common_head": (1, 0)}
_ADAMW_CASES = {}


def _adamw_case(n):
    """Inputs and float64 references (without and with the clip coefficient) of one length, computed once and never written to.
    The gradient values are bf16 numbers, so one reference serves both gradient dtypes."""
    if n not in _ADAMW_CASES:
        c = dict(master=rnd(n, seed=1, scale=0.02).float(), m=rnd(n, dtype=F32, seed=2, scale=1e-2),
                 v=rnd(n, dtype=F32, seed=3, scale=1e-2).abs(), grad=rnd(n, seed=4), coef=torch.tensor([0.37], device=DEV))  # fmt: skip
        c["ref"] = {clip: R.adamw(c["master"], c["m"], c["v"], c["grad"], c["coef"] if clip else torch.ones(1, device=DEV),
                                  *_adam_args(ADAM), F64) for clip in (False, True)}  # fmt: skip
        _ADAMW_CASES[n] = c
    return _ADAMW_CASES[n]


@pytest.mark.parametrize("g_f32,p_f32", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("layout", list(ADAMW_LAYOUTS))
def test_adamw_heads_tails_and_layouts(layout, g_f32, p_f32):
    """kai0_adamw's scalar head, vectors and scalar tail: n = 1 and 3 (the head clamped to n), 5 (head 1 + one vector with every
    stream one element in), 255, 1027 (one block's 256 vectors + a 3-element tail), 4099; every stream 16-byte aligned, every
    stream one element in (a common head of 3), f32 streams one element in with aligned 16-bit ones (no common head: the scalar
    form; with f32 gradient and model copy this is `one_in` again); every (grad, param) dtype pair; clip coefficient absent and
    from device memory.  Moments and master within the float64 bound, the model copy exactly the rounded master, guard bands."""
    off32, off16 = ADAMW_LAYOUTS[layout]
    gdt, goff = (F32, off32) if g_f32 else (BF16, off16)
    pdt, poff = (F32, off32) if p_f32 else (BF16, off16)
    for n in ADAMW_N:
        c = _adamw_case(n)
        grad = Out((n,), gdt, init=c["grad"], off=goff).t
        for clip in (False, True):
            o = dict(master=Out((n,), F32, init=c["master"], off=off32), m=Out((n,), F32, init=c["m"], off=off32),
                     v=Out((n,), F32, init=c["v"], off=off32), param=Out((n,), pdt, off=poff))  # fmt: skip
            call("kai0_adamw", P(o["master"].t), P(o["m"].t), P(o["v"].t), P(grad), g_f32, P(o["param"].t), p_f32, n, *_adam_args(ADAM),
                 P(c["coef"]) if clip else None)
            torch.cuda.synchronize()
            what = f"B adamw n={n} {layout} g_f32={g_f32} p_f32={p_f32} clip={clip}"
            for k in ("master", "m", "v", "param"):
                o[k].check(f"{what}.{k}")
            for k in ("master", "m", "v"):
                within(o[k].t, c["ref"][clip][k], f"{what}.{k}")
            exact(o["param"].t, o["master"].t.to(pdt), f"{what} model copy")


@pytest.mark.parametrize("g_f32", [0, 1])
def test_adamw_rows_past_the_grid_cap(g_f32):
    """16 384 blocks, one row each a trip; 16 384 + 37 rows of 8 elements.  Bit-identical to kai0_adamw on the same buffers
    (kai0hip.h), idle rows untouched, row_active set exactly for the rows that saw a gradient."""
    rows, rl = 16384 + 37, 8
    n = rows * rl
    k = dict(ADAM, wd=1e-10, lr=2.5e-5)
    master0 = rnd(n, seed=1, scale=0.02).float()
    grad = rnd(rows, rl, dtype=F32 if g_f32 else BF16, seed=4)
    live = torch.rand(rows, generator=torch.Generator().manual_seed(5)).to(DEV) < 0.5
    live[-37:] = torch.tensor([i % 2 == 0 for i in range(37)], device=DEV)
    grad[~live] = 0
    grad[~live, ::2] = -0.0
    grad = grad.reshape(-1)
    coef = torch.tensor([0.37], device=DEV)
    active = {"big": torch.zeros(rows, dtype=torch.uint8, device=DEV), "small": torch.zeros(rows, dtype=torch.uint8, device=DEV)}
    which = iter(("big", "small"))

    def new():
        o = dict(master=Out((n,), F32, init=master0), m=Out((n,), F32, fill=0.0), v=Out((n,), F32, fill=0.0), param=Out((n,), BF16, init=master0.to(BF16)))
        o["_active"] = active[next(which)]
        return o

    def launch(lo, hi, o):
        e = lo * rl
        call("kai0_adamw_rows", P(o["master"].t[e:]), P(o["m"].t[e:]), P(o["v"].t[e:]), P(grad[e:]), g_f32, P(o["param"].t[e:]), 0, hi - lo, rl,
             P(o["_active"][lo:]), *_adam_args(k), P(coef))

    big, small = new(), new()
    launch(0, rows, big)
    for lo in range(0, rows, 8192):
        launch(lo, min(rows, lo + 8192), small)
    dense = dict(master=Out((n,), F32, init=master0), m=Out((n,), F32, fill=0.0), v=Out((n,), F32, fill=0.0), param=Out((n,), BF16))
    call("kai0_adamw", P(dense["master"].t), P(dense["m"].t), P(dense["v"].t), P(grad), g_f32, P(dense["param"].t), 0, n, *_adam_args(k), P(coef))
    torch.cuda.synchronize()
    for key in ("master", "m", "v", "param"):
        for o in (big, small, dense):
            o[key].check(f"adamw_rows.{key}")
        exact(big[key].t, dense[key].t, f"adamw_rows.{key} vs kai0_adamw")
        exact(small[key].t, big[key].t, f"adamw_rows.{key} sliced")
    assert torch.equal(active["big"].bool(), live) and torch.equal(active["small"].bool(), live)
    assert bool((big["m"].t.view(rows, rl)[~live] == 0).all())
    for rows, rl in ROWS_SHAPES:
        for off in (0, 1):
            _adamw_rows_small(rows, rl, g_f32, off, k, coef)


# (19, 12): scalar scan, vector update; (19, 6): scalar throughout; (5, 2056): a second trip of the 2048-element scan stride and of the
# 1024-element update stride
ROWS_SHAPES = [(37, 8), (19, 12), (19, 6), (5, 2056)]


def _adamw_rows_small(rows, rl, g_f32, off, k, coef):
    """kai0_adamw_rows on [rows][rl] with every stream `off` elements past a 16-byte boundary (1: no vector scan, no vector
    update) against kai0_adamw on clones: all four outputs equal, every third row idle (zeros and -0.0 for a gradient) keeps its
    bytes and its clear flag, the other rows get their flag."""
    n, gdt = rows * rl, F32 if g_f32 else BF16
    master0 = rnd(n, seed=1, scale=0.02).float()
    live = torch.tensor([i % 3 != 1 for i in range(rows)], device=DEV)
    g = rnd(rows, rl, dtype=gdt, seed=4)
    g[~live] = 0
    g[~live, ::2] = -0.0
    grad = Out((n,), gdt, init=g.reshape(-1), off=off).t
    init = dict(master=master0, m=torch.zeros(n, device=DEV), v=torch.zeros(n, device=DEV), param=master0.to(BF16))
    sparse, dense = ({key: Out((n,), t.dtype, init=t, off=off) for key, t in init.items()} for _ in range(2))
    active = torch.zeros(rows, dtype=torch.uint8, device=DEV)
    call("kai0_adamw_rows", P(sparse["master"].t), P(sparse["m"].t), P(sparse["v"].t), P(grad), g_f32, P(sparse["param"].t), 0, rows, rl,
         P(active), *_adam_args(k), P(coef))
    call("kai0_adamw", P(dense["master"].t), P(dense["m"].t), P(dense["v"].t), P(grad), g_f32, P(dense["param"].t), 0, n, *_adam_args(k), P(coef))
    torch.cuda.synchronize()
    what = f"adamw_rows {rows}x{rl} off={off}"
    for key, t in init.items():
        sparse[key].check(f"{what}.{key}")
        dense[key].check(f"{what}.{key} (dense)")
        exact(sparse[key].t, dense[key].t, f"{what}.{key} vs kai0_adamw")
        assert torch.equal(sparse[key].t.view(rows, rl)[~live], t.view(rows, rl)[~live]), f"{what}.{key}: an idle row changed"
    assert not torch.equal(sparse["master"].t.view(rows, rl)[live], master0.view(rows, rl)[live])
    assert torch.equal(active.bool(), live), what


# =================================================================================================== B. the rest
def test_embed_grad_many_occurrences():
    """B = 3, T = 200, D = 136, 50 ids: 600 tokens = three blocks' worth of the j += 256 scans and 19 bitmap words; ids whose
    first and last occurrence are more than 256 positions apart, one id filling a whole sample, two ids that never occur (their
    rows keep what was there).  The gradient is read through a row offset, a row stride and a batch stride."""
    Bt, T, D, V, S_ld, ld, row0 = 3, 200, 136, 50, 208, 144, 3
    scale = 136**0.5
    tok = R.embed_tokens(Bt, T, V).to(DEV)
    dout = rnd(Bt, S_ld, ld, seed=1)
    dt = Out((V, D), BF16, fill=7.0)
    call("kai0_embed_grad", P(dout), P(tok), P(dt.t), Bt, T, D, scale, S_ld * ld, row0, ld)
    dt.check("embed_grad")
    ref, occ = R.embed_grad(dout[:, row0 : row0 + T, :D].reshape(Bt * T, D), tok, V, scale, F64)
    assert int((~occ).sum()) == 2 and bool((dt.t[~occ] == 7.0).all()), "rows of ids that do not occur were touched"
    within(dt.t[occ], R.Res(ref.value[occ], ref.terms[occ]), "B embed_grad")


def test_embed_gather_second_column_trip():
    """D = 2056: embed_gather_kernel's `c0 += 2048` loop makes a second trip; one f32 product rounded once: exact against torch."""
    Bt, T, D, V, S_ld, ld, row0 = 2, 9, 2056, 50, 16, 2064, 3
    table = rnd(V, D, seed=1)
    tok = torch.randint(0, V, (Bt, T), generator=torch.Generator().manual_seed(2)).to(DEV)
    out = Out((Bt, S_ld, ld), BF16, fill=3.0)
    call("kai0_embed_gather", P(table), P(tok), P(out.t), Bt, T, D, D**0.5, S_ld * ld, row0, ld)
    out.check("embed_gather")
    want = torch.full((Bt, S_ld, ld), 3.0, dtype=BF16, device=DEV)
    want[:, row0 : row0 + T, :D] = (table[tok].float() * R.f32c(D**0.5)).to(BF16)
    exact(out.t, want, "embed_gather")


def test_gated_bwd_and_copy_rows_second_column_trip():
    """D = 2056: the `c0 += 2048` loops of gated_bwd_kernel and copy_rows_kernel make a second trip (one thread, 8 columns)."""
    B, rpb, D = 2, 5, 2056
    dout, y, gate = rnd(B * rpb, D, seed=1), rnd(B * rpb, D, seed=2), rnd(B, D, seed=3)
    dy, dgate = Out((B * rpb, D), BF16), Out((B, D), BF16)
    call("kai0_gated_bwd", P(dout), P(y), P(gate), P(dy.t), P(dgate.t), B * rpb, rpb, D)
    dy.check("gated_bwd.dy")
    dgate.check("gated_bwd.dgate")
    want_dy, ref = R.gated_bwd(dout, y, gate, rpb, F64)
    exact(dy.t, want_dy, "gated_bwd.dy")
    within(dgate.t, ref["dgate"], "B gated_bwd.dgate")
    out = Out((B * rpb, D), BF16)
    call("kai0_gated_fwd", P(dout), P(y), P(gate), P(out.t), B * rpb, rpb, D)
    out.check("gated_fwd")
    exact(out.t, R.gated_fwd_exact(dout, y, gate, rpb), "gated_fwd D=2056")


@pytest.mark.parametrize("D", [2056, 136, 8])
def test_copy_rows_with_offsets_and_strides(D):
    B, rows, s_rows, d_rows, sld, dld, sr0, dr0 = 2, 5, 9, 11, D + 8, D + 24, 2, 4
    src = rnd(B, s_rows, sld, seed=1)
    dst = Out((B, d_rows, dld), BF16, fill=3.0)
    call("kai0_copy_rows_bf16", P(src), P(dst.t), B, rows, D, s_rows * sld, sr0, sld, d_rows * dld, dr0, dld)
    dst.check("copy_rows")
    want = torch.full((B, d_rows, dld), 3.0, dtype=BF16, device=DEV)
    want[:, dr0 : dr0 + rows, :D] = src[:, sr0 : sr0 + rows, :D]
    exact(dst.t, want, "copy_rows_bf16")


@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("N", [8, 520])
@pytest.mark.parametrize("M", [1, 3, 1023, 4100])
def test_colsum_direct(M, N, out_f32):
    """kai0_colsum_bf16 on its own: fewer rows than waves, the 4-rows-in-flight loop and its remainder, a second column block
    (N = 520 > 512), ld > N."""
    from kai0_amd.ops import COLSUM_BLOCKS

    ld = N + 16
    dy = rnd(M, ld, seed=M + N)
    scratch = Out((COLSUM_BLOCKS, N), F32, fill=0.0)
    out = Out((N,), F32 if out_f32 else BF16)
    call("kai0_colsum_bf16", P(dy), M, N, ld, P(scratch.t), COLSUM_BLOCKS, P(out.t), out_f32)
    out.check("colsum.out")
    scratch.check("colsum.scratch")
    within(out.t, R.colsum(dy, N, F64)["out"], f"B colsum M={M} N={N} f32={out_f32}")


def test_reduce_partials_batch_equals_single_launches():
    """kai0_reduce_partials_batch, the form the training step launches, on 33 items: a second launch of the 32-item split.  The
    items cycle through (blocks, ncols, f32 out, first column, ld) = (1, 8, f32, 0, 8): the smallest; (17, 70, bf16, 8, 96): a
    partial second 64-column block, one pass of the 16-row-group loop and a remainder, columns read from inside a wider row;
    (512, 520, f32, 0, 520): nine column blocks.  Every output equals kai0_reduce_partials on the same item bit for bit."""
    import ctypes as C

    from kai0_amd import _lib

    shapes = [(1, 8, 1, 0, 8), (17, 70, 0, 8, 96), (512, 520, 1, 0, 520)]
    parts, outs, single, fields = [], [], [], []
    for i in range(33):
        blocks, ncols, f32, col0, ld = shapes[i % 3]
        part = rnd(blocks, ld, dtype=F32, seed=i)
        parts.append(part)
        outs.append(Out((ncols,), F32 if f32 else BF16))
        single.append(Out((ncols,), F32 if f32 else BF16))
        fields.append((part.data_ptr() + 4 * col0, blocks, ncols, ld, f32))
    items = (_lib.ReduceItem * 33)(*[_lib.ReduceItem(src, P(o.t), ld, blocks, ncols, f32, 0) for (src, blocks, ncols, ld, f32), o in zip(fields, outs)])
    call("kai0_reduce_partials_batch", C.addressof(items), 33)
    for (src, blocks, ncols, ld, f32), o in zip(fields, single):
        call("kai0_reduce_partials", src, blocks, ncols, ld, P(o.t), f32)
    torch.cuda.synchronize()
    for i, (o, s) in enumerate(zip(outs, single)):
        o.check(f"reduce_partials_batch item {i}")
        s.check(f"reduce_partials item {i}")
        exact(o.t, s.t, f"reduce_partials_batch item {i} vs kai0_reduce_partials")


@pytest.mark.parametrize("n", [5, 8, 13, 1000 + 5])
def test_add_bf16_add_f32_small(n):
    a, b = rnd(n, seed=1), rnd(n, seed=2)
    af, bf = a.float(), b.float()
    o16, o32 = Out((n,), BF16), Out((n,), F32)
    call("kai0_add_bf16", P(a), P(b), P(o16.t), n)
    call("kai0_add_f32", P(af), P(bf), P(o32.t), n)
    o16.check("add_bf16")
    o32.check("add_f32")
    exact(o16.t, (a.float() + b.float()).to(BF16), "add_bf16")
    exact(o32.t, af + bf, "add_f32")
