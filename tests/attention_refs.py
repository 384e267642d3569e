"""Float64 references, per-element error bounds and f32 emulations for the attention kernels: kai0_attn_fwd (csrc/attention.hip: the
resident, one-pass online and two-pass forms), kai0_attn_combine, kai0_attn_bwd_dq2 / kai0_attn_bwd_dq (csrc/attn_bwd.hip) and
kai0_attn_decode (csrc/attn_decode.hip).  A plain helper module like tests/skinny_refs.py: nothing here touches the HIP library,
everything runs on whichever device its inputs live on.

Exact logits.  The kernels round the logits twice, s = bf16(bf16(q k) * scale); a reference that misses that rounding by one bf16 ulp
is off by a factor e^(2^-7 |s|) in P.  The inputs here make it reproducible bit for bit: Q and K hold only {-1, 0, +1}, so every q k
is an integer of magnitude <= HD <= 256 — exact in f32 under any summation order and exact in bf16 (8 significant bits) — and
bf16(n * scale) is ONE f32 multiply and ONE rounding, which `exact_logits` performs in torch f32.  Kernel, emulation and reference
therefore hold the same bf16 logits for every HD and every scale.  V, dO and O are ordinary seeded N(0, 1) bf16 values.

Families (`inputs`): `count` (Q = 0: every logit 0, l = number of visible keys, V with a spike of 64 at column key % HD: one key too
many or too few moves one output column by 64 / count), `integer` (scale HD^-0.5, logit std ~ 1) and `peaked` (scale 4 HD^-0.5 and
planted keys that copy a growing prefix of a query row tile after tile, so that row's running maximum moves at every key tile, and
for another row a dominant key in the first tile only).

Masks (`codes`) are int32 codes placed by hand; the rule is the kernels' own: key j is visible to folded row r iff j < Sk and
kcode[j] <= qcode[q0 + r / H].

One formula per operation for either working dtype: float64 gives the reference and the bound, float32 the emulation with the
header's rounding points, torch.exp for __expf and 64-key tiles in the kernel's order.  The kernels are never used to choose a constant.

The bounds, derived.  U32 = 2^-23 (twice the rounding error of one f32 operation), UBF = 2^-8 (one bf16 rounding, relative), SIG_ERR
= 2e-7 (absolute error of __expf for results in [0, 1], tests/streaming_refs.py), TINY = 2^-126.  Per row: A the visible key set, m
the maximum logit, e_j = exp(s_j - m), L = sum e >= 1 (the maximum contributes exactly 1), p = e / L, T_d = sum_j p_j |v_jd|, and
`moves` the number of rescales exp(m_old - m_new) the form applies to its running state (`moves` below).

  forward O   computed = (sum_j bf16(e~_j) a_j v_j) / (sum_j e~_j a_j), e~ = e + d, |d| <= SIG_ERR, a_j the product of the rescale
              factors applied after tile(j), each with absolute error SIG_ERR and <= 1.
                store              UBF |O|
                bf16(P)            rounding e~ (one-pass) or e~ / L (two-pass, resident, decode) is UBF relative per key: UBF T; the
                                   rounded value is itself off by the other terms, hence UBF (1 + UBF) T
                f32 arithmetic     a sum of <= Sk products in any order, (Sk - 1) half-ulps at twice that allowance (gemm_refs),
                                   one multiply per rescale, the division by L, the sum L itself (relative (|A| - 1) / 2 ulp, and
                                   |A| <= Sk, moving O by at most that times T) and 1 / L: (Sk + moves + 4) U32 T
                __expf             d O = sum_j d_j v_j / L - O sum_j d_j / L: SIG_ERR (sum_A |v_jd| + |A| T_d) / L for the
                                   exponentials themselves and the same again for every rescale (its error multiplies a state of at
                                   most sum_A |v| resp. |A| at the old maximum), plus one for the final normalisation: (moves + 2)
  forward P   UBF p + SIG_ERR (1 + p |A| (1 + moves)) / L + U32 p (|A| + 2) + TINY — streaming_refs.softmax_fwd's argument: d p / d e
              = 1 / L, d p / d L = -p / L, L off by SIG_ERR |A| for its exponentials and by the same again per rescale of pass 1.
  lse         lse = m + log L.  U32 (|m| + |log L| + |lse|) for the f32 log, add and store, (|A| U32 + SIG_ERR (moves + 1) |A|) / L for
              the error of L through d log L = d L / L, and a REQUIREMENT of 2^-12 on __logf: the consumers round exp(s - lse) to bf16
              (2^-8 relative) and lse may contribute at most 1 / 16 of that.  Rows with no visible key hold exactly +inf.
  combine     O = sum_s w_s O_s, w_s = exp(lse_s - m) / W, W = sum_t exp(lse_t - m) >= 1: UBF |O| for the store, (parts + 3) U32
              sum_s w_s |O_s| for the f32 products, sum, 1 / W and the scaling, and 2 SIG_ERR sum_s |O_s| / W for __expf (each weight
              off by SIG_ERR / W directly and by at most as much again through W, since sum_s w_s |O_s| <= sum_s |O_s|).
  backward    lse, O and (stored form) P are inputs; every stage is held against the f64 value computed FROM WHAT THE LAUNCH ITSELF
              STORED for the stage before (the rowsq_out argument of skinny_refs), so each bound stays at round-off size:
                Pout = bf16(exp(s - lse))         UBF p + SIG_ERR + U32 |s - lse| p + TINY  (the f32 subtraction moves p by U32 |s -
                                                  lse| p; with lse = +inf or a hidden key exactly 0)
                dS = bf16((P (dP - D)) scale)     P scale HD U32 (|dO| |V|^T + sum_d |dO O|) for the two f32 dot products of HD exact
                                                  products, 3 U32 |dS| for the subtraction and two multiplies, UBF |dS| for the store
                dQ = bf16(dS K)                   Sk U32 |dS| |K| + UBF |dQ| + TINY
              Columns Sk .. ldp of P and dS are exact zeros.

`moves` counts the rescales of the running SUM: they enter O only through L (the |A| T_d part of the __expf term, and the P and lse
bounds).  The O accumulator itself is rescaled by the one-pass form alone: for the other forms the sum_A |v| part of the __expf term
and the f32 term take 0 instead.  `moves` is 0 for the resident form and for decode (the whole row's maximum is known before the first exponential); for the one-pass
form the number of 64-key tiles at which the row's running maximum changes (the block-uniform maximum of attention.hip, made
uniform over the lane groups every tile); for the two-pass form pass 1 keeps one running maximum per lane group (keys 4 g .. 4 g + 3
of every 16) and merges the four with two more rescales: the largest count among the groups, plus 2.

Worst err / bound of the f32 emulations over every case of the tables below (tests/test_attention_refs_cpu.py prints them):
  forward O      resident 0.837, one-pass 0.722, two-pass 0.885, decode 0.820
  forward P      resident 0.995, two-pass 0.994
  lse            resident 0.006, one-pass 0.005, two-pass 0.004
  backward       Pout 0.995, dS 0.995 (recompute) / 0.995 (stored P), dQ 0.994 / 0.994
  combine        0.995
(UBF is the LARGEST relative error of one bf16 rounding, reached just above a power of two: a ratio close to 1 on a stored bf16 value is
its final rounding alone, and the one-pass O, whose P rounding term is an allowance the f64 reference cannot locate, sits lower.)
"""

import functools

import torch

from gemm_refs import SENTINEL, TINY, U32, UBF, assert_within, worst  # noqa: F401  (re-exported for the tests)
from streaming_refs import SIG_ERR

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
INT_MAX = 2**31 - 1
INF = float("inf")
NAN = float("nan")
TILE = 64
LSE_REQ = 2.0**-12
AB_KC_MAX = 2048  # csrc/attn_bwd.hip: the recompute form takes at most this many keys
KC_LDS_MAX = 2048  # csrc/attention.hip: up to here the key codes sit in LDS and the one-pass form walks a live-tile list


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ case tables
HD_SMALL = (16, 72, 128)  # <2,128,*>: 72 pads the second 64-wide sub-tile
HD_LARGE = (136, 256)  # <4,256,*>: 136 pads the last one
SK_EDGES = (1, 63, 64, 65, 128, 129, 200, 256, 257, 321)
ROW_CASES = ((1, 1), (3, 8), (16, 8), (17, 8), (50, 8))  # (Sq, H): 1 row, a wave and a half, one block, a ragged second block, 400
ROWS_EDGE = (17, 8)  # the row case of the Sk-edge list: 136 folded rows
SK_ROWS = (65, 200)  # the Sk of the row-case list
FAMILIES = ("count", "integer", "peaked")
FORMS = {  # form -> (HDs, largest Sk of the edge list, emulation / moves kind)
    "F1": (HD_SMALL, 256, "resident"),
    "F2": (HD_SMALL, 321, "online"),
    "F3": (HD_SMALL, 321, "twopass"),
    "F4": (HD_LARGE, 321, "online"),
    "F5": (HD_LARGE, 321, "twopass"),
}
BWD_HD = (16, 72, 136, 256)
BWD_SK = (1, 63, 65, 129, 200, 257)
DEAD_KINDS = ("dead_first", "dead_mid", "dead_last", "dead_all")
TILE_KINDS = DEAD_KINDS + ("single",)  # every one of them runs in every forward form at each Sk of SK_TILE_KINDS (136 rows)
SK_TILE_KINDS = (200, 321)  # four and six key tiles, the last one ragged (8 and 1 keys)
DEC_NO_CODES = (33, 257)  # decode launches with qcode = kcode = NULL, on every grid
COMBINE_PARTS, COMBINE_HD, COMBINE_ROWS = (1, 3, 8), (8, 72, 256), (1, 33, 400)
DEC_SK = (1, 31, 32, 33, 127, 128, 129, 255, 257, 1024)
DEC_GRIDS = ((1, 2), (4, 15), (3, 21))  # (batch, Sq) at H = 8: ceil(8 Sq / 16) x batch = 1, 32 and 33 — both sides of the fine / coarse switch


def mask_kinds(Sk):
    """The mask of each of the two batch entries of a joint-style case with Sk keys: hand-placed codes for entry 0; for entry 1 a
    whole dead tile / a tile with one visible key where Sk has the tiles for it, chosen by Sk.  (That choice alone does not reach every
    kind in every list: fwd_cases adds each kind of TILE_KINDS explicitly.)"""
    nt = (Sk + TILE - 1) // TILE
    if nt == 1:
        return ("mixed", "single")
    if nt == 2:
        return ("mixed", ("dead_first", "dead_last", "single")[Sk % 3])
    return ("mixed", ("dead_first", "dead_mid", "dead_last", "single")[Sk % 4])


def bwd_cases():
    """(HD, Sq, H, Sk, kinds) of either backward form: every Sk x HD x row case, ldp = round_up(Sk, 8)."""
    return [(HD, Sq, H, Sk, mask_kinds(Sk)) for Sk in BWD_SK for HD in BWD_HD for Sq, H in ROW_CASES]


def fwd_cases(form):
    """(HD, Sq, H, Sk, q0, kinds) of a forward form: every Sk edge at 136 rows, every row case at Sk 65 and 200, every kind of
    TILE_KINDS at Sk 200 (and 321 beyond the resident form), one case without codes, and (non-resident forms) the long case."""
    hds, sk_max, _ = FORMS[form]
    out = []
    for i, Sk in enumerate(s for s in SK_EDGES if s <= sk_max):
        for j, HD in enumerate(hds):
            Sq, H = ROWS_EDGE
            q0 = Sk - Sq if (i + j) % 2 and Sk >= Sq else 0
            out.append((HD, Sq, H, Sk, q0, mask_kinds(Sk)))
    for Sk in SK_ROWS:
        for j, (Sq, H) in enumerate(ROW_CASES):
            for HD in hds:
                for q0 in {0, max(Sk - Sq, 0)}:
                    out.append((HD, Sq, H, Sk, q0, mask_kinds(Sk)))
    for Sk in (s for s in SK_TILE_KINDS if s <= sk_max):
        for j, kind in enumerate(TILE_KINDS):
            out.append((hds[j % len(hds)], 17, 8, Sk, 0, ("mixed", kind)))
    out.append((hds[1], 17, 8, 200, 0, None))
    if form != "F1":
        out.append((hds[0], 24, 1, 2049, 0, ("mixed", "dead_mid")))
    return out


# ------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def ternary(*shape, seed):
    return (torch.randint(0, 3, shape, generator=_gen(seed)) - 1).to(BF16)


def normal(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed)).to(BF16)


@functools.lru_cache(maxsize=None)
def inputs(family, B, rows, Sk, HD, seed=0):
    """(q [B, rows, HD], k [B, Sk, HD], v [B, Sk, HD], scale) on the CPU; treat as read-only (cached)."""
    scale = HD**-0.5
    k = ternary(B, Sk, HD, seed=seed + 1)
    v = normal(B, Sk, HD, seed=seed + 2)
    if family == "count":
        q = torch.zeros(B, rows, HD, dtype=BF16)
        key = torch.arange(Sk)
        v = v.clone()
        v[:, key, key % HD] += 64.0
        return q, k, v, scale
    q = ternary(B, rows, HD, seed=seed + 3)
    if family == "integer":
        return q, k, v, scale
    assert family == "peaked"
    nt = (Sk + TILE - 1) // TILE
    k = k.clone()
    for t in range(nt):
        n = -(-HD * (t + 1) // nt)  # the planted key of tile t copies the first n elements of the row and is 0 beyond
        for row, off in ((0, 3), (rows - 1, 7)):
            j = t * TILE + off
            if j < Sk:
                k[:, j] = 0
                k[:, j, :n] = q[:, row, :n]
    if rows > 2 and Sk > 11:
        k[:, 11] = q[:, 1]  # row 1: the dominant key in the first tile only
    return q, k, v, 4.0 * scale


def codes(kinds, nq, Sk):
    """(qcode [B, nq], kcode [B, Sk]) int32 for one mask kind per batch entry; None -> (None, None)."""
    if kinds is None:
        return None, None
    nt = (Sk + TILE - 1) // TILE
    qs, ks = [], []
    for b, kind in enumerate(kinds):
        i, j = torch.arange(nq), torch.arange(Sk)
        qc = (i + b) % 3
        qc[i % 7 == 3] = -1  # sees nothing
        kc = (j * 5 + b) % 3
        kc[j % 13 == 6] = INT_MAX  # isolated padded slots
        dead = {"dead_first": [0], "dead_mid": [nt // 2], "dead_last": [nt - 1], "dead_all": list(range(nt))}.get(kind, [])
        for t in dead:
            kc[t * TILE : (t + 1) * TILE] = INT_MAX
        if kind == "single":  # a tile with exactly one visible key (code 0: visible to every query but -1)
            t = nt // 2
            kc[t * TILE : (t + 1) * TILE] = INT_MAX
            kc[min(t * TILE + 37, Sk - 1)] = 0
        qs.append(qc)
        ks.append(kc)
    return torch.stack(qs).to(torch.int32), torch.stack(ks).to(torch.int32)


def visible(qcode, kcode, B, rows, Sk, H, q0=0, *, strict=False, shift=0, device="cpu"):
    """bool [B, rows, Sk]: kcode[j] <= qcode[q0 + r / H].  strict / shift: planted defects (< for <=; row r + shift's position)."""
    if qcode is None:
        return torch.ones(B, rows, Sk, dtype=torch.bool, device=device)
    pos = q0 + torch.clamp((torch.arange(rows, device=qcode.device) + shift) // H, max=qcode.shape[1] - 1 - q0)
    qc = qcode[:, pos].unsqueeze(-1).long()
    kc = kcode[:, :Sk].unsqueeze(1).long()
    return (kc < qc) if strict else (kc <= qc)


def exact_logits(q, k, scale):
    """bf16(bf16(q k) * scale) as the kernels hold it (module docstring), bf16 [B, rows, Sk].  The integers are formed in f64."""
    n = (q.to(F64) @ k.to(F64).transpose(-1, -2)).to(F32)
    assert float(n.abs().max()) <= 256 and bool((n.to(BF16).to(F32) == n).all())
    return (n * torch.tensor(scale, dtype=F32, device=n.device)).to(BF16)


def padded(x, rows_to=None, pad=8, fill=NAN):
    """x [B, R, W] -> storage [B, rows_to or R + pad, W + pad] holding `fill` outside the corner."""
    B, R, W = x.shape
    st = torch.full((B, rows_to or R + pad, W + pad), fill, dtype=x.dtype, device=x.device)
    st[:, :R, :W] = x
    return st


def assert_untouched(store, what, rows, width):
    """Everything of `store` [.., R, W] outside [.., :rows, :width] still holds the sentinel."""
    masked = store.clone()
    masked[..., :rows, :width] = SENTINEL
    assert bool((masked == SENTINEL).all()), f"{what}: {int((masked != SENTINEL).sum())} elements written outside the window"


# ------------------------------------------------------------------------------------------------ forward
def _stored(x, e):
    """Bound of a value x computed to within e and stored as bf16: the rounded number is at most |x| + e (gemm_refs.Chain.round_bf16)."""
    return e + UBF * (x.abs() + e) + TINY


def _tiles(x, fill):
    """x [B, R, Sk] -> [B, R, nt, 64] padded with `fill`."""
    Sk = x.shape[-1]
    nt = (Sk + TILE - 1) // TILE
    pad = torch.full((*x.shape[:-1], nt * TILE - Sk), fill, dtype=x.dtype, device=x.device)
    return torch.cat([x, pad], -1).reshape(*x.shape[:-1], nt, TILE)


def _changes(tmax):
    """tmax [.., nt]: number of tiles at which the running maximum changes."""
    run = torch.cummax(tmax, -1).values
    prev = torch.cat([torch.full_like(run[..., :1], -INF), run[..., :-1]], -1)
    return (run > prev).sum(-1, keepdim=True).to(F64)


def moves(S, kind):
    """The rescales of `kind` per row (module docstring), f64 [B, R, 1], from the masked exact logits S (-inf where hidden)."""
    if kind in ("resident", "decode"):
        return torch.zeros(*S.shape[:-1], 1, dtype=F64, device=S.device)
    t = _tiles(S, -INF)
    if kind == "online":
        return _changes(t.amax(-1))
    assert kind == "twopass"
    g = t.reshape(*t.shape[:-1], 4, 4, 4).amax((-3, -1))  # [.., nt, 4 lane groups]
    return torch.stack([_changes(g[..., i]) for i in range(4)]).amax(0) + 2


def fwd_ref(s, vis, v, kind):
    """f64 reference and bounds of one forward: s bf16 exact logits [B, R, Sk], vis bool, v [B, Sk, HD].  Returns a dict of (ref, bound)
    pairs for O [B, R, HD], P [B, R, Sk] and lse [B, R] (bound +inf - inf-free: rows without a visible key have ref +inf, bound 0)."""
    S = torch.where(vis, s.to(F64), torch.full_like(s, -INF, dtype=F64))
    m = S.amax(-1, keepdim=True)
    live = m > -INF
    m0 = torch.where(live, m, torch.zeros_like(m))
    e = torch.where(vis, torch.exp(S - m0), torch.zeros_like(S))
    L = e.sum(-1, keepdim=True)
    Lc = L.clamp_min(1.0)  # live rows have L >= 1: the maximum contributes exactly 1
    p = e / Lc
    V = v.to(F64)
    O, T = p @ V, p @ V.abs()
    A = vis.sum(-1, keepdim=True).to(F64)
    SA = vis.to(F64) @ V.abs()
    Sk = s.shape[-1]
    mv = moves(S, kind)  # rescales of the running sum L
    mo = mv if kind == "online" else torch.zeros_like(mv)  # rescales of the O accumulator: the one-pass form only
    bO = _stored(O, (UBF * (1 + UBF) + (Sk + mo + 4) * U32) * T + SIG_ERR * ((mo + 2) * SA + (mv + 2) * A * T) / Lc)
    bP = UBF * p + SIG_ERR * (1 + p * A * (1 + mv)) / Lc + U32 * p * (A + 2) + TINY
    bP = torch.where(vis, bP, torch.full_like(bP, TINY))  # a hidden key's probability is exactly 0
    logL = torch.log(Lc)
    lse = torch.where(live, m0 + logL, torch.full_like(m, INF))
    bl = U32 * (m0.abs() + logL.abs() + (m0 + logL).abs()) + (A * U32 + SIG_ERR * (mv + 1) * A) / Lc + LSE_REQ
    return {"O": (O, bO), "P": (p, bP), "lse": (lse.squeeze(-1), bl.squeeze(-1)), "moves": mv}


def assert_lse(out, ref, bound, what):
    """lse rows without a visible key hold exactly +inf; the others are inside the bound.  Returns the worst err / bound."""
    dead = torch.isinf(ref)
    assert bool((out[dead] == INF).all()), f"{what}: a row without a visible key does not hold +inf"
    if bool(dead.all()):
        return 0.0
    return assert_within(out[~dead].reshape(1, -1), ref[~dead].reshape(1, -1), bound[~dead].reshape(1, -1), what)


def fwd_emulate(s, vis, v, kind, *, ldp=None, defect=None):
    """The f32 evaluation in the kernel's order -> (O bf16 [B, R, HD], P bf16 [B, R, ldp] or None, lse f32 [B, R]).  kind: online (one
    pass, running maximum, P~ = bf16(exp(s - m_run)), rescale when the maximum moved), twopass (pass 1: tile-wise row max / sum; pass
    2: P = bf16(exp(s - m) / l)), resident / decode (the same with the whole row at once).  P (exact forms) has the zero columns Sk
    .. ldp.  defect: a planted error for tests/test_attention_refs_cpu.py."""
    B, R, Sk = s.shape
    HD = v.shape[-1]
    St = _tiles(torch.where(vis, s.to(F32), torch.full_like(s, -INF, dtype=F32)), -INF)
    nt = St.shape[-2]
    Vt = torch.cat([v.to(F32), torch.zeros(B, nt * TILE - Sk, HD, device=v.device)], 1).reshape(B, nt, TILE, HD)
    tile_keys = _tiles(vis.any(1, keepdim=True).to(F32), 0.0).sum(-1)[:, 0]  # [B, nt]: keys of a tile visible to anybody
    zero = torch.zeros(B, R, 1, device=s.device)

    def pv(pt, t):
        if defect == "swap_p_blocks" and t == nt - 1:  # two 16-key blocks of P exchanged against V
            pt = torch.cat([pt[..., 16:32], pt[..., :16], pt[..., 32:]], -1)
        return pt.to(BF16).to(F32) @ Vt[:, t]

    m = torch.full((B, R, 1), -INF, device=s.device)
    l, o = zero.clone(), torch.zeros(B, R, HD, device=s.device)
    if kind == "online":
        last = m
        for t in range(nt):
            st = St[..., t, :]
            if defect == "skip_single":  # a tile with exactly one visible key taken for dead
                st = torch.where((tile_keys[:, t] == 1).view(B, 1, 1), torch.full_like(st, -INF), st)
            tmax = st.amax(-1, keepdim=True)
            mn = torch.maximum(m, tmax)
            lv = mn > -INF
            alpha = torch.where(lv, torch.exp(m - mn), torch.ones_like(m))
            e = torch.where(lv, torch.exp(st - mn), torch.zeros_like(st))
            l = l * alpha + e.sum(-1, keepdim=True)
            if defect == "skip_rescale" and t == nt - 1:  # the last tile's rescale of O left out
                alpha = torch.ones_like(alpha)
            o = o * alpha + pv(e, t)
            m, last = mn, tmax
        inv = torch.where(l > 0, 1.0 / l, zero)
        o = o * inv
        mm = last if defect == "lse_last_tile_max" else m
        lse = torch.where(l > 0, mm + torch.log(l), torch.full_like(l, INF))
        return o.to(BF16), None, lse.squeeze(-1)
    def absorb(m, l, mo, lo):  # (m, l) joined with a partial (mo, lo) at its own maximum: one rescale each, as the kernel's merge
        mn = torch.maximum(m, mo)
        lv = mn > -INF
        return torch.where(lv, mn, m), torch.where(lv, l * torch.exp(m - mn) + lo * torch.exp(mo - mn), l)

    if kind == "twopass":  # pass 1: one running (max, sum) per lane group (keys 4 g .. 4 g + 3 of every 16), merged g ^ 1 then g ^ 2
        Sg = St.reshape(B, R, nt, 4, 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(B, R, nt, 4, 16)
        m, l = torch.full((B, R, 4), -INF, device=s.device), torch.zeros(B, R, 4, device=s.device)
        for t in range(nt):
            st = Sg[:, :, t]
            mn = torch.maximum(m, st.amax(-1))
            lv = mn > -INF
            l = torch.where(lv, l * torch.exp(m - mn) + torch.exp(st - mn.unsqueeze(-1)).sum(-1), l)
            m = torch.where(lv, mn, m)
        m2, l2 = absorb(m[..., 0::2], l[..., 0::2], m[..., 1::2], l[..., 1::2])
        m, l = absorb(m2[..., :1], l2[..., :1], m2[..., 1:], l2[..., 1:])
    else:  # resident / decode: the whole row at once
        st = St.reshape(B, R, -1)
        mn = st.amax(-1, keepdim=True)
        lv = mn > -INF
        m, l = torch.where(lv, mn, m), torch.where(lv, torch.exp(st - mn).sum(-1, keepdim=True), l)
    inv = torch.where(l > 0, 1.0 / l, zero)
    lse = torch.where(l > 0, m + torch.log(l), torch.full_like(l, INF))
    P = torch.zeros(B, R, nt * TILE, dtype=BF16, device=s.device)
    for t in range(nt):
        pt = torch.where(m > -INF, torch.exp(St[..., t, :] - m) * inv, torch.zeros_like(St[..., t, :]))
        P[..., t * TILE : (t + 1) * TILE] = pt.to(BF16)
        o = o + pv(pt, t)
    return o.to(BF16), (P[..., : ldp or Sk] if kind != "decode" else None), lse.squeeze(-1)


# ------------------------------------------------------------------------------------------------ backward
def bwd_inputs(family, B, rows, Sk, HD, kinds, H, seed=0):
    """Everything a backward launch reads, on the CPU: q, k, v, scale, codes, the visibility (qcode[r / H]: no q0), exact logits, dO,
    and from the f64 forward O (bf16), lse (f32) and P (bf16: what the two-pass forward would have stored)."""
    q, k, v, scale = inputs(family, B, rows, Sk, HD, seed)
    qcode, kcode = codes(kinds, -(-rows // H), Sk)
    vis = visible(qcode, kcode, B, rows, Sk, H)
    s = exact_logits(q, k, scale)
    ref = fwd_ref(s, vis, v, "resident")
    return dict(q=q, k=k, v=v, scale=scale, qcode=qcode, kcode=kcode, vis=vis, s=s, dO=normal(B, rows, HD, seed=seed + 4),
                O=ref["O"][0].to(BF16), lse=ref["lse"][0].to(F32), P=ref["P"][0].to(BF16))


def bwd_p_ref(s, vis, lse):
    """(ref, bound) of Pout = bf16(exp(s - lse)) from the GIVEN f32 lse [B, R]."""
    l = lse.to(F64).unsqueeze(-1)
    ok = vis & torch.isfinite(l)
    d = torch.where(ok, s.to(F64) - torch.where(torch.isfinite(l), l, torch.zeros_like(l)), torch.zeros_like(s, dtype=F64))
    p = torch.where(ok, torch.exp(d), torch.zeros_like(d))
    bound = torch.where(ok, UBF * p + SIG_ERR + U32 * d.abs() * p + TINY, torch.full_like(p, TINY))  # hidden: exactly 0
    return p, bound


def bwd_ds_ref(P, dO, O, v, scale):
    """(ref, bound) of dS = bf16((P (dP - D)) scale) from the STORED P [B, R, Sk]."""
    HD = v.shape[-1]
    p, do, o, V = P.to(F64), dO.to(F64), O.to(F64), v.to(F64)
    sc = float(torch.tensor(scale, dtype=F32))
    dP = do @ V.transpose(-1, -2)
    D = (do * o).sum(-1, keepdim=True)
    dS = p * (dP - D) * sc
    e_dot = HD * U32 * (do.abs() @ V.abs().transpose(-1, -2) + (do * o).abs().sum(-1, keepdim=True))
    return dS, _stored(dS, p * sc * e_dot + 3 * U32 * dS.abs())


def bwd_dq_ref(dS, k):
    """(ref, bound) of dQ = bf16(dS K) from the STORED dS [B, R, Sk]."""
    ds, K = dS.to(F64), k.to(F64)
    dQ = ds @ K
    return dQ, _stored(dQ, dS.shape[-1] * U32 * (ds.abs() @ K.abs()))


def bwd_emulate(s, vis, v, k, dO, O, lse, scale, ldp, *, P=None, defect=None):
    """f32 emulation of attn_bwd_dq_kernel -> (P bf16 [B, R, ldp], dS bf16 [B, R, ldp], dQ bf16 [B, R, HD]); P given: the stored-P form
    (P is passed through), else the recompute form, which walks the live tiles only and zero-fills the dead ones.  Outputs start as
    SENTINEL."""
    B, R, Sk = s.shape
    HD = v.shape[-1]
    rc = P is None
    nt = (Sk + TILE - 1) // TILE
    pad = lambda x: torch.cat([x.to(F32), torch.zeros(B, nt * TILE - Sk, HD, device=x.device)], 1).reshape(B, nt, TILE, HD)  # noqa: E731
    Vt, Kt = pad(v), pad(k)
    St = _tiles(torch.where(vis, s.to(F32), torch.full_like(s, -INF, dtype=F32)), -INF)
    live = _tiles(vis.any(1, keepdim=True).to(F32), 0.0).sum(-1)[:, 0] > 0  # [B, nt]
    D = (dO.to(F32) * O.to(F32)).sum(-1, keepdim=True)
    if defect == "neighbour_D":
        D = torch.roll(D, 1, 1)
    sc = torch.tensor(scale, dtype=F32, device=s.device)
    Pout = torch.full((B, R, nt * TILE), SENTINEL, dtype=BF16, device=s.device)
    dS = Pout.clone()
    dq = torch.zeros(B, R, HD, device=s.device)
    Pin = None if rc else torch.cat([P.to(F32), torch.zeros(B, R, nt * TILE - P.shape[-1], device=s.device)], -1)
    lse3 = lse.to(F32).unsqueeze(-1)
    for t in range(nt):
        cols = slice(t * TILE, (t + 1) * TILE)
        on = live[:, t].view(B, 1, 1) if rc else torch.ones(B, 1, 1, dtype=torch.bool, device=s.device)
        if rc:
            pt = torch.where(St[..., t, :] > -INF, torch.exp(St[..., t, :] - lse3), torch.zeros_like(St[..., t, :])).to(BF16)
        else:
            pt = Pin[..., cols].to(BF16)
        dP = dO.to(F32) @ Vt[:, t].transpose(-1, -2)
        ds = ((pt.to(F32) * (dP - D)) * sc).to(BF16)
        fill = SENTINEL if defect == "no_zero_fill" else 0.0
        Pout[..., cols] = torch.where(on, pt, torch.full_like(pt, fill))
        dS[..., cols] = torch.where(on, ds, torch.full_like(ds, fill))
        if not (defect == "dq_missing_tile" and t == nt - 1):
            dq = dq + torch.where(on, ds.to(F32) @ Kt[:, t], torch.zeros_like(dq))
    return Pout[..., :ldp], dS[..., :ldp], dq.to(BF16)


# ------------------------------------------------------------------------------------------------ combine
def combine_inputs(parts, rows, HD, seed=0):
    """(O parts bf16 [parts, rows, HD], lse f32 [parts, rows]): lse ~ 3 N(0, 1), rows near +90 and -90, some rows +inf in one part,
    some in all parts."""
    Op = normal(parts, rows, HD, seed=seed + 1)
    lse = 3.0 * torch.randn(parts, rows, generator=_gen(seed + 2))
    r = torch.arange(rows)
    lse[:, r % 5 == 1] += 90.0
    lse[:, r % 5 == 2] -= 90.0
    lse[(r % parts), r] = torch.where(r % 3 == 0, torch.tensor(INF), lse[(r % parts), r])
    lse[:, r % 11 == 4] = INF
    return Op, lse.to(F32)


def _combine(Op, lse, dt, defect=None):
    fin = lse < INF
    l = lse.to(dt)
    m = torch.where(fin, l, torch.full_like(l, -INF)).amax(0, keepdim=True)
    if defect == "no_max":
        m = torch.zeros_like(m)
    w = torch.where(fin, torch.exp(l - torch.where(m > -INF, m, torch.zeros_like(m))), torch.zeros_like(l))
    if defect == "inf_weight_one":
        w = torch.where(fin, w, torch.ones_like(w))
    return w, w.sum(0)


def combine_ref(Op, lse):
    """(ref, bound) f64 [rows, HD]."""
    w, W = _combine(Op, lse, F64)
    Wc = W.clamp_min(1.0).unsqueeze(-1)
    o = Op.to(F64)
    wn = (w / W.clamp_min(1.0)).unsqueeze(-1)
    O, T = (wn * o).sum(0), (wn * o.abs()).sum(0)
    return O, _stored(O, (Op.shape[0] + 3) * U32 * T + 2 * SIG_ERR * o.abs().sum(0) / Wc)


def combine_emulate(Op, lse, defect=None):
    w, W = _combine(Op, lse, F32, defect)
    acc = (w.unsqueeze(-1) * Op.to(F32)).sum(0)
    inv = torch.where(W > 0, 1.0 / W, torch.zeros_like(W))
    return (acc * inv.unsqueeze(-1)).to(BF16)


# ------------------------------------------------------------------------------------------------ checks shared by the CPU and GPU tests
def check_fwd(ref, O, P, lse, what, Sk):
    """Every output a forward produced against `ref` (fwd_ref); P [B, R, ldp] with exact zeros in columns Sk .. ldp.  Rows without a
    visible key: O exactly 0, lse exactly +inf.  Returns {"O" / "P" / "lse": worst err / bound}."""
    w = {"O": assert_within(O, *ref["O"], "O " + what)}
    dead = torch.isinf(ref["lse"][0])
    assert bool((O[dead] == 0).all()), f"O {what}: a row without a visible key is not zero"
    if P is not None:
        w["P"] = assert_within(P[..., :Sk], *ref["P"], "P " + what)
        assert bool((P[..., Sk:] == 0).all()), f"P {what}: columns Sk .. ldp are not exact zeros"
    if lse is not None:
        w["lse"] = assert_lse(lse, *ref["lse"], "lse " + what)
    return w


def check_bwd(d, Pout, dS, dQ, what, rc):
    """A backward launch's outputs, each stage against the f64 value of what the launch stored for the stage before.  d: bwd_inputs
    (on the outputs' device).  Returns {"Pout" / "dS" / "dQ": worst err / bound}."""
    Sk = d["s"].shape[-1]
    w = {}
    if rc:
        w["Pout"] = assert_within(Pout[..., :Sk], *bwd_p_ref(d["s"], d["vis"], d["lse"]), "Pout " + what)
        assert bool((Pout[..., Sk:] == 0).all()), f"Pout {what}: columns Sk .. ldp are not exact zeros"
    w["dS"] = assert_within(dS[..., :Sk], *bwd_ds_ref(Pout[..., :Sk], d["dO"], d["O"], d["v"], d["scale"]), "dS " + what)
    assert bool((dS[..., Sk:] == 0).all()), f"dS {what}: columns Sk .. ldp are not exact zeros"
    w["dQ"] = assert_within(dQ, *bwd_dq_ref(dS[..., :Sk], d["k"]), "dQ " + what)
    return w
