"""Input builders, float64 references and per-element error bounds for the streaming kernels (element-wise, norm, reduction and
optimizer kernels of csrc/elementwise.hip, csrc/norm.hip, csrc/optim.hip).  A plain helper module like tests/tiny.py: nothing here
touches the HIP library, everything runs on whichever device its inputs live on.

One formula per operation.  Every operation below is written ONCE, after its description in include/kai0hip.h, as a function of a
working dtype `dt`:

  dt = float64  the reference.  No intermediate rounding: the header's inner bf16 rounding points are left out on purpose (a
                reference that rounded inside would sit on the other side of a rounding boundary from a correct f32 kernel once in
                2^16 elements and then be off by a whole bf16 ulp); they are accounted for in the bound instead.
  dt = float32  the "plain fp32 evaluation with the header's rounding points" that tests/test_streaming_refs_cpu.py holds against
                the bound to calibrate it.  The kernels are never used to choose a constant.

Each function returns {output name: Res(value, terms, extra)}:
  value  the result in `dt` (not yet rounded to the stored dtype; `store()` does that for the f32 emulation),
  terms  the sum of the absolute values of the addends of that element's own expression (what an f32 evaluation's rounding
         errors scale with, cancellation or not),
  extra  further absolute allowances that follow from the number formats / the header, spelled out where they are added:
         one bf16 ulp (2^-7 relative, the same allowance the stored result gets) of an intermediate that the header rounds to
         bf16, propagated to the output, and the header's 2e-7 absolute error of the fast sigmoid / exponential times
         |d out / d sigma|.

bound = ulp(stored dtype) * |ref| + c * terms + extra + 2^-126      ulp = 2^-7 (bf16), 2^-23 (f32);  c = C0 = 2^-18 unless noted
and nothing may fall outside it (no outlier share).
"""

import math

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
# Coefficient of `terms`: 64 f32 half-ulps.  Not raised for any operation: the fp32 emulations of test_streaming_refs_cpu.py reach at
# most 0.498 of the bound where the result is stored in bf16 (0.5 is the final rounding alone: half an ulp against the one-ulp
# allowance) and at most 0.114 (silu_bwd; everything else <= 0.05) where it is stored in f32.
C0 = 2.0**-18
SIG_ERR = 2e-7       # common.h: |error| of the exp2/rcp sigmoid (and of __expf on [0, 1] results)
ULP_BF16 = 2.0**-7   # one bf16 ulp (relative, at most): the allowance per bf16 rounding, for the stored result and for inner ones alike
TINY = 2.0**-126     # smallest normal f32 / bf16: below it results may be flushed to zero or lose bits (absolute floor of every bound)
GUARD = 64           # sentinel elements on both sides of every output
SENTINEL = -24576.0  # exactly representable in bf16 and f32, far from every result
INT_MAX = 2**31 - 1


class Res:
    __slots__ = ("value", "terms", "extra")

    def __init__(self, value, terms, extra=None):
        self.value, self.terms, self.extra = value, terms, extra


def f32c(v: float) -> float:
    """The value a C `float` argument / constant has."""
    return float(torch.tensor(v, dtype=F32))


def rb(t):
    """Round to bf16 and back (a bf16-typed intermediate of the header); identity for the float64 reference."""
    return t if t.dtype == F64 else t.to(BF16).to(t.dtype)


def store(value, dtype):
    """The stored result of the f32 emulation."""
    return value.to(dtype)


def bound(res: Res, out_dtype, c: float = C0):
    ulp = 2.0**-7 if out_dtype == BF16 else 2.0**-23
    b = ulp * res.value.abs() + c * res.terms + TINY
    if res.extra is not None:
        b = b + res.extra
    return b


def worst_ratio(out, res: Res, out_dtype=None, c: float = C0) -> float:
    """max over elements of |out - ref| / bound; inf if any element is outside a zero bound or is not finite where ref is."""
    out_dtype = out.dtype if out_dtype is None else out_dtype
    err = (out.to(F64) - res.value.to(F64)).abs()
    bnd = bound(res, out_dtype, c).to(F64)
    ok = err <= bnd  # False for NaN
    if bool(ok.all()):
        r = err / bnd.clamp_min(1e-300)
        r = torch.where(err == 0, torch.zeros_like(r), r)
        return float(r.max()) if r.numel() else 0.0
    return float("inf")


def assert_within(out, res: Res, what: str, c: float = C0, limit: float = 1.0) -> float:
    r = worst_ratio(out, res, c=c)
    if not r <= limit:
        err = (out.to(F64) - res.value.to(F64)).abs()
        bnd = bound(res, out.dtype, c).to(F64)
        bad = ~(err <= bnd)
        idx = torch.nonzero(bad.reshape(-1))[:4].reshape(-1).tolist()
        fin = torch.where(bad & torch.isfinite(err), err / bnd.clamp_min(1e-300), torch.zeros_like(err))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound (worst finite error/bound "
                             f"{float(fin.max()):.3g}); first flat indices {idx}, got {out.reshape(-1)[idx].tolist()}, "
                             f"want {res.value.reshape(-1)[idx].tolist()}")
    return r


# ------------------------------------------------------------------------------------------------ input builders
def randn(*shape, dtype=BF16, seed=0, scale=1.0, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(device)


HARD_KINDS = ("zero", "const 100", "const 100, one element +1 bf16 ulp", "100 + N(0,1)", "1e4 N(0,1)", "1e-4 N(0,1)", "N(0,1)")


def hard_rows(reps: int, D: int, seed=0, device="cpu"):
    """bf16 [7 * reps][D]; row i is of kind HARD_KINDS[i % 7], so any 7 consecutive rows hold every kind."""
    n = randn(7 * reps, D, dtype=F32, seed=seed)
    x = torch.empty(7 * reps, D)
    x[0::7] = 0.0
    x[1::7] = 100.0
    x[2::7] = 100.0
    x[2::7, (3 * D) // 4] = 100.5  # bf16 has 8 significant bits: one ulp at 100 is 0.5
    x[3::7] = 100.0 + n[3::7]
    x[4::7] = 1e4 * n[4::7]
    x[5::7] = 1e-4 * n[5::7]
    x[6::7] = n[6::7]
    return x.to(BF16).to(device)


GELU_SPECIALS = (0.0, -0.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4)


def gelu_points(n: int, device="cpu"):
    """bf16 [n]: a deterministic grid over [-12, 12] followed by the specials (twice): the GELU tails where exp2 saturates.
    Stops at |x| = 1e4: beyond ~2e19 this library and torch's own backward both form 0 * inf."""
    sp = torch.tensor(GELU_SPECIALS * 2)
    grid = torch.linspace(-12.0, 12.0, n - sp.numel())
    return torch.cat([grid, sp]).to(BF16).to(device)


def mix_gelu_points(base, device=None):
    """`base` (flat bf16, N(0,1)-like) with gelu_points written over its head, its middle and its last 4096 elements."""
    x = base.clone()
    n = x.numel()
    k = min(4096, n // 8 * 8)
    pts = gelu_points(k, x.device)
    x[:k] = pts
    x[n - k :] = pts
    x[n // 2 : n // 2 + k] = pts
    return x


def softmax_rows(rows: int, Sk: int, ld: int, seed=0, device="cpu"):
    """bf16 [rows][ld] logits: row r % 5 == 0 all equal, 1 equal at 3e4, 2 a spread of +-80 around the middle, else 3 N(0,1);
    the padding columns [Sk, ld) hold 6e4 (larger than every logit: a kernel that reads them shows it)."""
    s = randn(rows, ld, dtype=F32, seed=seed, scale=3.0)
    s[0::5] = 1.5
    s[1::5] = 3e4
    g = torch.Generator().manual_seed(seed + 1)
    for r in range(2, rows, 5):
        s[r, :Sk] = torch.linspace(-80.0, 80.0, Sk)[torch.randperm(Sk, generator=g)]
    s[:, Sk:] = 6e4
    return s.to(BF16).to(device)


def codes_from_pad_att(pad, att):
    """kai0hip.h kai0_softmax_mask_fwd: kcode = pad ? cumsum(att) : INT_MAX, qcode = pad ? cumsum(att) : -1 (int32)."""
    cum = torch.cumsum(att.to(torch.int32), dim=1).to(torch.int32)
    q = torch.where(pad, cum, torch.full_like(cum, -1))
    k = torch.where(pad, cum, torch.full_like(cum, INT_MAX))
    return q.contiguous(), k.contiguous()


def allowed_mask(qcode, kcode, Sq: int, Sk: int, q0: int):
    """bool [B][Sq][Sk]: kcode[b][j] <= qcode[b][q0 + s] (None codes: everything allowed)."""
    return kcode[:, None, :Sk] <= qcode[:, q0 : q0 + Sq, None]


def softmax_case(ld: int, masked: bool, seed=0, device="cpu"):
    """Section B softmax input: 2 batch entries x 37 rows (H = 1), Sk = ld - 5, q0 = Sk - 37.  masked: key codes in {0 (one key, in
    the ragged last chunk), 1, 2, INT_MAX}, query codes in {-1 (sees nothing), 0 (sees that one key), 1, 2}.
    -> (scores [2][37][ld], qcode, kcode (int32 [2][Sk]) or None, allowed [2][37][Sk] or None)"""
    rows, Sk = 37, ld - 5
    scores = softmax_rows(2 * rows, Sk, ld, seed=seed).view(2, rows, ld).to(device)
    if not masked:
        return scores, None, None, None
    g = torch.Generator().manual_seed(seed + 7)
    kcode = torch.where(torch.rand(2, Sk, generator=g) < 0.1, INT_MAX, torch.randint(1, 3, (2, Sk), generator=g)).to(torch.int32)
    kcode[:, Sk - 3] = 0
    qcode = torch.randint(1, 3, (2, Sk), generator=g).to(torch.int32)
    q0 = Sk - rows
    qcode[:, q0 + 4] = -1   # rows 4 and 9 see nothing
    qcode[:, q0 + 9] = -1
    qcode[:, q0 + 6] = 0    # rows 6 and 11 see key Sk - 3 alone
    qcode[:, q0 + 11] = 0
    qcode, kcode = qcode.to(device), kcode.to(device)
    return scores, qcode, kcode, allowed_mask(qcode, kcode, rows, Sk, q0)


def embed_tokens(B: int, T: int, V: int, seed=0):
    """int64 [B][T] over a vocabulary of V: sample 1 is filled with id V - 2 alone; samples 0 and 2.. draw from ids 0 .. V - 4
    (8 to 9 occurrences each at B = 3, T = 200, V = 50 — one id owning a whole sample leaves the others 400 / 47 — and an id's
    first and last occurrence lie in different samples, more than T apart);
    ids V - 3 and V - 1 never occur."""
    g = torch.Generator().manual_seed(seed)
    k, free = V - 3, (B - 1) * T - 2 * (V - 3)
    mid = (torch.arange(free) % k)[torch.randperm(free, generator=g)]  # evenly spread over the ids, shuffled
    rest = torch.cat([torch.arange(k), mid, torch.arange(k)])  # every drawn id at the head of sample 0 and at the tail of the last
    tok = torch.empty(B, T, dtype=torch.int64)
    tok[1] = V - 2
    tok[[b for b in range(B) if b != 1]] = rest.view(B - 1, T)
    return tok


# ------------------------------------------------------------------------------------------------ norms
def _eps(eps, dt):
    return torch.tensor(f32c(eps), dtype=dt)


def rmsnorm_fwd(x, w, eps, dt, mod=None, rpb=1):
    """y = (x * rstd) * (1 + w)  or, with mod [B][3 D] f32, (x * rstd) * (1 + scale_b) + shift_b;  rstd = rsqrt(mean(x^2) + eps)."""
    X = x.to(dt)
    D = X.shape[-1]
    rstd = torch.rsqrt((X * X).mean(-1, keepdim=True) + _eps(eps, dt).to(X.device))
    if mod is None:
        W = w.to(dt)
        y = (X * rstd) * (1 + W)
        ty = X.abs() * rstd * (1 + W.abs())
    else:
        M = mod.to(dt).repeat_interleave(rpb, 0)[: X.shape[0]]
        sc, sh = M[:, :D], M[:, D : 2 * D]
        y = (X * rstd) * (1 + sc) + sh
        ty = X.abs() * rstd * (1 + sc.abs()) + sh.abs()
    return {"y": Res(y, ty), "rstd": Res(rstd[:, 0], rstd[:, 0].abs())}


def layernorm_fwd(x, w, b, eps, dt):
    """y = (x - mean) * rstd * w + b, two-pass statistics."""
    X, W, Bv = x.to(dt), w.to(dt), b.to(dt)
    mean = X.mean(-1, keepdim=True)
    d = X - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + _eps(eps, dt).to(X.device))
    y = d * rstd * W + Bv
    a = X.abs() + mean.abs()  # addends of x - mean
    ty = a * rstd * W.abs() + Bv.abs()
    # rstd = (var + eps)^-1/2: d rstd = rstd^3 / 2 * d var, and var's addends d^2 carry the error of d = x - mean twice
    trstd = rstd + rstd**3 * (d.abs() * a).mean(-1, keepdim=True)
    return {"y": Res(y, ty), "mean": Res(mean[:, 0], X.abs().mean(-1)), "rstd": Res(rstd[:, 0], trstd[:, 0])}


def rmsnorm_bwd(dy, x, w, rstd, dres, dt, mod=None, rpb=1, dgate=None):
    """xh = x * rstd; dxh = dy * (1 + w | scale_b); s = mean(dxh * xh); dx = rstd * (dxh - xh * s) + dres;
    dw = sum_rows dy * xh  (adaRMS: dmod[b] = [sum dy * xh | sum dy | dgate] over the rows of b)."""
    DY, X, R = dy.to(dt), x.to(dt), rstd.to(dt)[:, None]
    rows, D = X.shape
    if mod is None:
        cw = 1 + w.to(dt)
    else:
        cw = 1 + mod.to(dt)[:, :D].repeat_interleave(rpb, 0)
    xh = X * R
    dxh = DY * cw
    s = (dxh * xh).mean(-1, keepdim=True)
    dx = R * (dxh - xh * s)
    tdx = R * (dxh.abs() + xh.abs() * (dxh * xh).abs().mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(dt)
        tdx = tdx + dres.to(dt).abs()
    out = {"dx": Res(dx, tdx)}
    p = DY * xh
    if mod is None:
        out["dw"] = Res(p.sum(0), p.abs().sum(0))
    else:
        B = rows // rpb
        dsc, dsh = p.view(B, rpb, D).sum(1), DY.view(B, rpb, D).sum(1)
        dg = dgate.to(dt) if dgate is not None else torch.zeros_like(dsc)
        out["dmod"] = Res(torch.cat([dsc, dsh, dg], 1),
                          torch.cat([p.abs().view(B, rpb, D).sum(1), DY.abs().view(B, rpb, D).sum(1), dg.abs()], 1))
    return out


def layernorm_bwd(dy, x, w, mean, rstd, dres, dt):
    """xh = (x - mean) * rstd; dxh = dy * w; dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)) + dres; dw = sum dy * xh; db = sum dy.
    xh's own addends are x * rstd and mean * rstd: `xa` = (|x| + |mean|) * rstd stands for |xh| in every term."""
    DY, X, W = dy.to(dt), x.to(dt), w.to(dt)
    M, R = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (X - M) * R
    xa = (X.abs() + M.abs()) * R
    dxh = DY * W
    s1 = dxh.mean(-1, keepdim=True)
    s2 = (dxh * xh).mean(-1, keepdim=True)
    dx = R * (dxh - s1 - xh * s2)
    tdx = R * (dxh.abs() + dxh.abs().mean(-1, keepdim=True) + xa * (dxh.abs() * xa).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(dt)
        tdx = tdx + dres.to(dt).abs()
    return {"dx": Res(dx, tdx), "dw": Res((DY * xh).sum(0), (DY.abs() * xa).sum(0)), "db": Res(DY.sum(0), DY.abs().sum(0))}


# ------------------------------------------------------------------------------------------------ softmax / rowdot
def softmax_fwd(scores, allowed, Sk, dt):
    """probs = softmax over the allowed columns j < Sk; 0 on masked and padding columns; a row that sees no key is all zeros.
    scores [..., ld]; allowed: bool broadcastable to [..., Sk] or None."""
    s = scores[..., :Sk].to(dt)
    if allowed is not None:
        s = torch.where(allowed, s, torch.full_like(s, float("-inf")))
    m = s.max(-1, keepdim=True).values
    live = m > float("-inf")
    e = torch.where(live, torch.exp(s - torch.where(live, m, torch.zeros_like(m))), torch.zeros_like(s))
    S = e.sum(-1, keepdim=True)
    p = torch.where(live, e / S.clamp_min(1e-30), torch.zeros_like(e))
    # __expf: absolute error SIG_ERR on every exponential (all in [0, 1]); p = e / S: d p / d e = 1 / S, d p / d S = -p / S
    extra = torch.where(live, SIG_ERR * (1 + p * Sk) / S.clamp_min(1e-30), torch.zeros_like(e))
    pad = scores.shape[-1] - Sk
    z = torch.zeros(*p.shape[:-1], pad, dtype=dt, device=p.device)
    return {"probs": Res(torch.cat([p, z], -1), torch.cat([p, z], -1), torch.cat([extra, z], -1))}


def softmax_bwd(probs, dprobs, Sk, scale, dt):
    """dscores = (p * (dp - sum_j p dp)) * scale over j < Sk (columns beyond read as zero, written as zero)."""
    P, DP = probs.to(dt).clone(), dprobs.to(dt).clone()
    P[..., Sk:] = 0
    DP[..., Sk:] = 0
    sc = f32c(scale)
    dot = (P * DP).sum(-1, keepdim=True)
    ds = (P * (DP - dot)) * sc
    t = (P.abs() * DP.abs() + P.abs() * (P * DP).abs().sum(-1, keepdim=True)) * abs(sc)
    return {"dscores": Res(ds, t)}


def rowdot(a, b, dt):
    p = a.to(dt) * b.to(dt)
    return {"out": Res(p.sum(-1), p.abs().sum(-1))}


# ------------------------------------------------------------------------------------------------ GELU family, SiLU
_BETA, _KAPPA = 0.7978845608028654, 0.044715


def _gelu_parts(x):
    """sigma(2u), 2u' and their products for u = beta (x + kappa x^3): gelu = x sigma, gelu' = sigma + x sigma (1 - sigma) 2u'."""
    u2 = 2 * _BETA * (x + _KAPPA * x**3)
    sig = torch.sigmoid(u2)
    du2 = 2 * _BETA * (1 + 3 * _KAPPA * x * x)
    return sig, du2


def gelu_fwd(x, dt):
    X = x.to(dt)
    sig, _ = _gelu_parts(X)
    y = X * sig
    return {"y": Res(y, y.abs(), SIG_ERR * X.abs())}


def _gelu_grad(X):
    sig, du2 = _gelu_parts(X)
    t2 = X * sig * (1 - sig) * du2
    g = sig + t2
    dsig = (1 + X * (1 - 2 * sig) * du2).abs()  # |d gelu' / d sigma|
    return g, sig.abs() + t2.abs(), dsig


def geglu_fwd(g, u, dt):
    """h = bf16( bf16(gelu_tanh(g)) * u )"""
    G, U = g.to(dt), u.to(dt)
    sig, _ = _gelu_parts(G)
    a = G * sig
    h = rb(a) * U
    # the inner bf16(gelu): one bf16 ulp of it, times |u|; the sigmoid's error times |d h / d sigma| = |g u|
    return {"h": Res(h, (a * U).abs(), ULP_BF16 * (a * U).abs() + SIG_ERR * (G * U).abs())}


def geglu_bwd(dh, g, u, dt):
    """du = bf16(dh * bf16(gelu_tanh(g)));  dg = bf16( bf16(dh * u) * gelu_tanh'(g) )"""
    DH, G, U = dh.to(dt), g.to(dt), u.to(dt)
    sig, _ = _gelu_parts(G)
    a = G * sig
    du = DH * rb(a)
    gp, tg, dsig = _gelu_grad(G)
    q = DH * U
    dg = rb(q) * gp
    return {"du": Res(du, (DH * a).abs(), ULP_BF16 * (DH * a).abs() + SIG_ERR * (DH * G).abs()),
            "dg": Res(dg, q.abs() * tg, ULP_BF16 * (q * gp).abs() + SIG_ERR * q.abs() * dsig)}


def gelu_bwd(dy, pre, dt):
    """dx = bf16(dy * gelu_tanh'(pre))"""
    DY, X = dy.to(dt), pre.to(dt)
    gp, tg, dsig = _gelu_grad(X)
    return {"dx": Res(DY * gp, DY.abs() * tg, SIG_ERR * DY.abs() * dsig)}


def gelu_saturated(x):
    """bool: where |x| >= 30 the sigmoid is exactly 0 or 1 in f32 and in f64 (its argument is beyond +-1900): gelu' is exactly 0 or
    1 and gelu exactly 0 or x, so the stored result is the one rounding of the reference — checked bit for bit there, because the
    SIG_ERR allowance, taken literally, grows with |x| 2u' and says nothing at the far tails."""
    return x.float().abs() >= 30.0


def silu_fwd(x, dt):
    X = x.to(dt)
    sig = torch.sigmoid(X)
    return {"y": Res(X * sig, (X * sig).abs(), SIG_ERR * X.abs())}


def silu_bwd(dy, x, dt):
    """dx = dy * (sg * (1 + x * (1 - sg)))"""
    DY, X = dy.to(dt), x.to(dt)
    sg = torch.sigmoid(X)
    t2 = X * sg * (1 - sg)
    dsig = (1 + X * (1 - 2 * sg)).abs()
    return {"dx": Res(DY * (sg + t2), DY.abs() * (sg + t2.abs()), SIG_ERR * DY.abs() * dsig)}


# ------------------------------------------------------------------------------------------------ gated residual, embedding, sums
def gated_fwd_exact(x, y, gate, rpb):
    """out = bf16(x + bf16(y * gate[b])): a product of two bf16 values is exact in f32, so every step is one IEEE rounding that
    torch's f32 arithmetic reproduces bit for bit."""
    gt = gate.float().repeat_interleave(rpb, 0)
    return (x.float() + (y.float() * gt).to(BF16).float()).to(BF16)


def gated_bwd(dout, y, gate, rpb, dt):
    """dy = bf16(dout * gate[b]) (one rounding: exact against torch);  dgate[b] = bf16(sum over the rows of b of dout * y)."""
    B, D = gate.shape
    dy = (dout.float() * gate.float().repeat_interleave(rpb, 0)).to(BF16)
    p = (dout.to(dt) * y.to(dt)).view(B, rpb, D)
    return dy, {"dgate": Res(p.sum(1), p.abs().sum(1))}


def embed_grad(dout_rows, tokens, V, scale, dt):
    """dtable[id] = bf16(sum over the occurrences of id of bf16(dout * scale)).  dout_rows: bf16 [B*T][D] (already gathered from
    the strided buffer).  The inner bf16(dout * scale) is a single f32 product rounded once: reproduced exactly.  -> (Res, occurs)"""
    v = (dout_rows.float() * f32c(scale)).to(BF16).to(dt)
    D = v.shape[-1]
    tok = tokens.reshape(-1).to(v.device)
    acc = torch.zeros(V, D, dtype=dt, device=v.device).index_add_(0, tok, v)
    tacc = torch.zeros(V, D, dtype=dt, device=v.device).index_add_(0, tok, v.abs())
    occurs = torch.zeros(V, dtype=torch.bool, device=v.device)
    occurs[tok] = True
    return Res(acc, tacc), occurs


def colsum(dy, N, dt):
    X = dy[:, :N].to(dt)
    return {"out": Res(X.sum(0), X.abs().sum(0))}


def sumsq(g, dt):
    s = (g.to(dt) ** 2).sum()
    return s


def sumsq_chain(n: int, is_f32: bool) -> int:
    """The longest chain of f32 additions one partial of kai0_sumsq goes through, from the kernel's structure: a thread adds V
    squares per vector (bf16, V = 8: squares exact in f32; f32, V = 4: every square also rounds once -> 2 V) over
    ceil(n / V / (4096 * 256)) grid-stride trips, one scalar tail element, 6 wave-shuffle steps and 4 wave partials in the block;
    the finishing launch adds 4096 / 256 = 16 block partials per thread, again 6 + 4, and `out[0] +=` is one more."""
    V = 4 if is_f32 else 8
    trips = -(-(n // V) // (4096 * 256))
    per = (2 * V if is_f32 else V) * trips
    return per + 1 + 6 + 4 + 16 + 6 + 4 + 1


# ------------------------------------------------------------------------------------------------ f32 glue
def flow_mix(noise, act, time, dt):
    """x_t = t * noise + (1 - t) * a;  u_t = noise - a"""
    N, A = noise.to(dt), act.to(dt)
    t = time.to(dt)[:, None]
    return {"xt": Res(t * N + (1 - t) * A, (t * N).abs() + ((1 - t) * A).abs()), "ut": Res(N - A, N.abs() + A.abs())}


def mse_fwd(u, v, dt):
    d = u.to(dt) - v.to(dt)
    # (u - v)^2: the difference's error 2^-24 (|u| + |v|) enters twice
    return {"loss": Res(d * d, d * d + 2 * d.abs() * (u.to(dt).abs() + v.to(dt).abs()))}


def mse_bwd(u, v, dl, dt):
    U, V, DL = u.to(dt), v.to(dt), dl.to(dt)
    return {"dv": Res(-2.0 * (U - V) * DL, 2.0 * (U.abs() + V.abs()) * DL.abs())}


def euler(x, v, dtv, dt):
    X, Vv = x.to(dt), v.to(dt)
    h = f32c(dtv)
    return {"x": Res(X + h * Vv, X.abs() + abs(h) * Vv.abs())}


def adamw(master, m, v, grad, coef, lr, b1, b2, eps, wd, bc1, bc2, dt):
    """kai0hip.h kai0_adamw (torch.optim.AdamW): g = grad * coef; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
    p = p (1 - lr wd) - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)."""
    lr, b1, b2, eps, wd, bc1, bc2 = (f32c(t) for t in (lr, b1, b2, eps, wd, bc1, bc2))
    g = grad.to(dt) * coef.to(dt)
    M = m.to(dt) * b1 + (1.0 - b1) * g
    tM = (m.to(dt) * b1).abs() + ((1.0 - b1) * g).abs()
    Vv = v.to(dt) * b2 + (1.0 - b2) * g * g
    P0 = master.to(dt) * (1.0 - f32c(lr * wd))
    step = (lr / bc1) * (M / (torch.sqrt(Vv) / math.sqrt(bc2) + eps))
    # the step inherits m's relative error (tM / |M|) and half of v's, which is a sum of non-negative addends
    tstep = (lr / bc1) * (tM / (torch.sqrt(Vv) / math.sqrt(bc2) + eps)) + step.abs()
    return {"master": Res(P0 - step, P0.abs() + tstep), "m": Res(M, tM), "v": Res(Vv, Vv.abs())}


# ------------------------------------------------------------------------------------------------ RoPE (bf16 torch restatement)
def rope_ref(x, pos, inv_freq, inverse=False):
    """modeling_gemma.py:149-194 in bf16: x [B, S, H, HD] bf16, pos [B, S]; every product and the sum rounded to bf16.
    The criteria of tests/test_kernels_gpu.py::test_rope apply (two libms: a handful of one-ulp flips of cos / sin)."""
    freqs = pos[:, :, None].float() * inv_freq[None, None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    cos, sin = emb.cos().to(BF16)[:, :, None, :], emb.sin().to(BF16)[:, :, None, :]
    if inverse:
        sin = -sin
    half = x.shape[-1] // 2
    rot = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return (x * cos) + (rot * sin)


def rope_close(y, ref):
    """-> (mismatch share, rel-L2); the project's limits are 2e-2 and 3e-3."""
    mism = (y != ref).float().mean().item()
    a, b = y.float(), ref.float()
    return mism, float((a - b).norm() / (b.norm() + 1e-12))


def im2col_ref(img, P):
    """cols [N * G * G][C * P * P], k = c * P * P + ky * P + kx (Conv2d weight order): a pure copy."""
    n, C, HW, _ = img.shape
    G = HW // P
    t = img.view(n, C, G, P, G, P).permute(0, 2, 4, 1, 3, 5)  # n, py, px, c, ky, kx
    return t.reshape(n * G * G, C * P * P).contiguous()
