"""The attention kernels — kai0_attn_fwd in its five instantiations, kai0_attn_combine, kai0_attn_bwd_dq2 / kai0_attn_bwd_dq in their four
and kai0_attn_decode in its two launch forms — held per element to the float64 bounds of tests/attention_refs.py on inputs whose
logits are exact (Q, K in {-1, 0, 1}), in the three families `count`, `integer` and `peaked` and under hand-placed mask codes.

Which instantiation a case reaches follows from the selection rules of kai0_attn_fwd (HD <= 128; Sk <= 256 and blocks x batch <= 512;
P given; online), attn_bwd_dq_launch (HD <= 128; rc) and kai0_attn_decode (query tiles x batch <= 32), and is named in each test.
Every operand sits in NaN-padded storage (columns HD .. ld, K / V rows from Sk on, Q rows past `rows`, the neighbours of a column
slice), every output in sentinel-filled storage whose padding must come back untouched; P and dS hold exact zeros in columns Sk ..
ldp; rows that see no key hold O = 0 and lse = +inf exactly.  References are computed on the GPU in f64 from the same tensors."""

import ctypes as C
import functools

import pytest
import torch

import attention_refs as R

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
WORST = {}  # (operation, form) -> worst err / bound seen (printed per test; profiles/HISTORY.md records a run)
PAD = 8


@pytest.fixture(scope="module")
def ops():
    from kai0_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module", autouse=True)
def module_end():
    """After the module's last test: print the worst err / bound per operation and form, and let go of the cached cases' GPU tensors."""
    yield
    for (op, form), w in sorted(WORST.items()):
        print(f"worst err / bound  {form:10s} {op:5s} {w:.3f}")
    fwd_case.cache_clear()
    torch.cuda.empty_cache()


def dev():
    return torch.device("cuda:0")


def note(form, what, w):
    for op, x in w.items():
        WORST[op, form] = max(WORST.get((op, form), 0.0), x)
    print(f"[{form}] {what}: worst err / bound " + ", ".join(f"{op} {x:.3f} (so far {WORST[op, form]:.3f})" for op, x in w.items()))


def sentinel(*shape, dtype=BF16):
    return torch.full(shape, R.SENTINEL, dtype=dtype, device=dev())


def kv_store(x):
    """K or V [B, Sk, HD] in NaN-padded storage: columns HD .. HD + 8, rows Sk .. round_up(Sk, 64) + 8."""
    return R.padded(x, rows_to=R.round_up(x.shape[1], 64) + PAD)


@functools.lru_cache(maxsize=None)
def fwd_case(family, HD, Sq, H, Sk, q0, kinds, B=2):
    """A forward case on the GPU: dense operands, codes, visibility, exact logits and the padded storages."""
    rows = Sq * H
    q, k, v, scale = (t.to(dev()) if torch.is_tensor(t) else t for t in R.inputs(family, B, rows, Sk, HD))
    qcode, kcode = (None if t is None else t.to(dev()) for t in R.codes(kinds, q0 + Sq, Sk))
    vis = R.visible(qcode, kcode, B, rows, Sk, H, q0, device=dev())
    return dict(q=q, k=k, v=v, scale=scale, qcode=qcode, kcode=kcode, vis=vis, s=R.exact_logits(q, k, scale), B=B, rows=rows, Sk=Sk,
                HD=HD, H=H, q0=q0, Qs=R.padded(q), Ks=kv_store(k), Vs=kv_store(v), refs={})


def ref_of(c, kind):
    if kind not in c["refs"]:
        c["refs"][kind] = R.fwd_ref(c["s"], c["vis"], c["v"], kind)
    return c["refs"][kind]


def entry(ref, e):
    return {k: tuple(t[e : e + 1] for t in v) for k, v in ref.items() if k != "moves"}


def launch_fwd(ops, c, form, *, want_p, want_lse, ldp, online=0, share=None):
    """One kai0_attn_fwd launch of a case and every check on what it wrote.  share = (entry, batch): `batch` entries that all read entry
    `entry`'s Q / K / V / codes through stride 0 and own only their O, P and lse (how a short-Sk case passes the 512-block rule)."""
    rows, Sk, HD, ld = c["rows"], c["Sk"], c["HD"], c["HD"] + PAD
    kind = R.FORMS[form][2]
    ref = ref_of(c, kind)
    if share is None:
        batch, sl, st = c["B"], slice(None), 1
    else:
        batch, sl, st = share[1], slice(share[0], share[0] + 1), 0
        ref = entry(ref, share[0])
    Qs, Ks, Vs = c["Qs"][sl], c["Ks"][sl], c["Vs"][sl]
    qcode, kcode = (None, None) if c["qcode"] is None else (c["qcode"][sl], c["kcode"][sl])
    O = sentinel(batch, rows + PAD, ld)
    P = sentinel(batch, rows + PAD, ldp) if want_p else None
    lse = sentinel(batch, rows + PAD, dtype=F32) if want_lse else None
    ops.attn_fwd(Qs, Ks, Vs, O, P, rows=rows, Sk=Sk, HD=HD, H=c["H"], q0=c["q0"], batch=batch, ldq=ld, ldk=ld, ldv=ld, ldo=ld,
                 ldp=ldp if want_p else 0, sQ=(st * Qs.stride(0), 0), sK=(st * Ks.stride(0), 0), sV=(st * Vs.stride(0), 0),
                 sO=(O.stride(0), 0), sP=P.stride(0) if want_p else 0, qcode=qcode, kcode=kcode,
                 code_ld=None if qcode is None else (st * qcode.stride(0), st * kcode.stride(0)), scale=c["scale"], lse=lse, online=online)
    torch.cuda.synchronize()
    what = f"{form} HD {HD} rows {rows} (H {c['H']}) Sk {Sk} q0 {c['q0']} batch {batch} ldp {ldp if want_p else '-'} lse {want_lse}"
    outs = [O[:, :rows, :HD], None if P is None else P[:, :rows], None if lse is None else lse[:, :rows]]
    if share is not None:  # every entry computed the same thing: bit for bit entry 0's, which is held to the bound
        for name, t in zip("O P lse".split(), outs):
            assert t is None or bool((t == t[:1]).logical_or(t.isnan() & t[:1].isnan()).all()), f"{name} {what}: batch entries differ"
        outs = [None if t is None else t[:1] for t in outs]
    w = R.check_fwd(ref, *outs, what, Sk)
    R.assert_untouched(O, "O " + what, rows, HD)
    if P is not None:
        R.assert_untouched(P, "P " + what, rows, ldp)
    if lse is not None:
        R.assert_untouched(lse.unsqueeze(1), "lse " + what, 1, rows)
    note(form, what, w)


def blocks_batch(rows):
    """The smallest batch at which a launch has more than 512 blocks."""
    return 512 // ((rows + 127) // 128) + 1


# ------------------------------------------------------------------------------------------------ forward: the five instantiations
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("form", list(R.FORMS))
def test_forward_form(ops, form, family):
    """F1 attn_fwd_kernel<2,128,4> (resident): HD <= 128, Sk <= 256, blocks x batch <= 512 — with and without P, with and without lse.
    F2 <2,128,-1> (one pass): HD <= 128, no P, Sk > 256 or more than 512 blocks.  F3 <2,128,0> (two passes): the same with P given, or
    online = 2 with lse.  F4 <4,256,-1>: HD > 128, no P.  F5 <4,256,0>: HD > 128, P given.  Cases: attention_refs.fwd_cases — every Sk
    edge at 136 rows, every row case at Sk 65 and 200 with both q0 and both ldp, a dead first / middle / last tile, all tiles dead and
    a one-key tile at Sk 200 (and 321: ragged last tiles), a case without codes and (F2 - F5) 33 tiles of keys whose codes are read
    from global memory.  F2 / F3 reach Sk <= 256 on 513-block grids whose entries share one entry's operands."""
    kind = R.FORMS[form][2]
    for i, (HD, Sq, H, Sk, q0, kinds) in enumerate(R.fwd_cases(form)):
        c = fwd_case(family, HD, Sq, H, Sk, q0, kinds)
        ldps = (R.round_up(Sk, 8), R.round_up(Sk, 64))
        if form == "F1":
            kw = dict(want_p=i % 2 == 0, want_lse=(i // 2) % 2 == 0)  # P + lse, lse, P, neither
        elif kind == "online":
            kw = dict(want_p=False, want_lse=i % 4 != 3)
        elif form == "F3" and i % 3 == 2:
            kw = dict(want_p=False, want_lse=True, online=2)
        else:
            kw = dict(want_p=True, want_lse=i % 2 == 0)
        for ldp in (ldps if Sk in R.SK_ROWS and kw["want_p"] else ldps[i % 2 : i % 2 + 1]):
            if form in ("F2", "F3") and Sk <= 256:
                for e in range(c["B"]):
                    launch_fwd(ops, c, form, ldp=ldp, share=(e, blocks_batch(c["rows"])), **kw)
            else:
                launch_fwd(ops, c, form, ldp=ldp, **kw)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("Sk,form", [(200, "F1"), (264, "F2")])
def test_forward_vision_tower_style(ops, Sk, form, family):
    """batch = 2 x 3 with batch_inner = 3: the heads are column slices of one [rows, 3 NH HD] q|k|v buffer (sQ2 = HD), no codes, HD = 72.
    Sk = 200: <2,128,4>; Sk = 264: <2,128,-1>.  The buffer's other columns and rows hold NaN; O is a column slice per head as well."""
    HD, NH, NI, rows = 72, 3, 2, Sk
    c = fwd_case(family, HD, rows, 1, Sk, 0, None, B=NI * NH)
    ld, ldo = 3 * NH * HD + PAD, NH * HD + PAD
    buf = torch.full((NI, rows + PAD, ld), R.NAN, dtype=BF16, device=dev())
    for part, x in enumerate((c["q"], c["k"], c["v"])):
        buf[:, :rows, part * NH * HD : (part + 1) * NH * HD] = x.reshape(NI, NH, rows, HD).transpose(1, 2).reshape(NI, rows, NH * HD)
    flat = buf.reshape(-1)
    O, lse = sentinel(NI, rows + PAD, ldo), sentinel(NI * NH, rows + PAD, dtype=F32)
    s1 = (buf.stride(0), HD)
    ops.attn_fwd(flat, flat[NH * HD :], flat[2 * NH * HD :], O, None, rows=rows, Sk=Sk, HD=HD, H=1, batch=NI * NH, batch_inner=NH, ldq=ld,
                 ldk=ld, ldv=ld, ldo=ldo, sQ=s1, sK=s1, sV=s1, sO=(O.stride(0), HD), scale=c["scale"], lse=lse)
    torch.cuda.synchronize()
    what = f"{form} vision-tower style Sk {Sk}"
    out = O[:, :rows, : NH * HD].reshape(NI, rows, NH, HD).transpose(1, 2).reshape(NI * NH, rows, HD)
    note(form, what, R.check_fwd(ref_of(c, R.FORMS[form][2]), out, None, lse[:, :rows], what, Sk))
    R.assert_untouched(O, "O " + what, rows, NH * HD)
    R.assert_untouched(lse.unsqueeze(1), "lse " + what, 1, rows)


# ------------------------------------------------------------------------------------------------ combine
@pytest.mark.parametrize("parts", R.COMBINE_PARTS)
def test_combine(ops, parts):
    """attn_combine_kernel: the lse-weighted mean of `parts` range outputs; +inf parts weigh nothing, a row that is +inf in every part comes
    out as zeros, lse near +-90 neither overflows nor vanishes (the maximum is subtracted)."""
    from kai0_amd import _lib

    for HD in R.COMBINE_HD:
        for rows in R.COMBINE_ROWS:
            Op, lse = (t.to(dev()) for t in R.combine_inputs(parts, rows, HD))
            lse_st = torch.full((parts, rows + 3), R.NAN, dtype=F32, device=dev())
            lse_st[:, :rows] = lse
            O = sentinel(rows + PAD, HD + PAD)
            _lib.call("kai0_attn_combine", Op.data_ptr(), lse_st.data_ptr(), O.data_ptr(), parts, rows, HD, HD + PAD, rows * HD, rows + 3,
                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            what = f"combine {parts} x {rows} x {HD}"
            note("combine", what, {"O": R.assert_within(O[:rows, :HD], *R.combine_ref(Op, lse), what)})
            assert bool((O[:rows, :HD][torch.isinf(lse).all(0)] == 0).all()), f"{what}: a row without any key is not zero"
            R.assert_untouched(O, what, rows, HD)


# ------------------------------------------------------------------------------------------------ backward
def launch_bwd(ops, family, HD, Sq, H, Sk, kinds, rc, *, expect_refusal=False):
    from kai0_amd import _lib

    B, rows, ld, ldp = 2, Sq * H, HD + PAD, R.round_up(Sk, 8)
    d = {k: (t.to(dev()) if torch.is_tensor(t) else t) for k, t in R.bwd_inputs(family, B, rows, Sk, HD, kinds, H).items()}
    dOs, Os, Qs, Ks, Vs = R.padded(d["dO"]), R.padded(d["O"]), R.padded(d["q"]), kv_store(d["k"]), kv_store(d["v"])
    lse = torch.full((B, rows + PAD), R.NAN, dtype=F32, device=dev())
    lse[:, :rows] = d["lse"]
    dS, dQ = sentinel(B, rows + PAD, ldp), sentinel(B, rows + PAD, ld)
    if rc:
        P = sentinel(B, rows + PAD, ldp)
    else:  # what the two-pass forward stores: the probabilities with zeros in columns Sk .. ldp; NaN in the rows nobody owns
        P = torch.full((B, rows + PAD, ldp), R.NAN, dtype=BF16, device=dev())
        P[:, :rows] = 0
        P[:, :rows, :Sk] = d["P"]
    stream = torch.cuda.current_stream().cuda_stream
    what = f"{'recompute' if rc else 'stored P'} <{2 if HD <= 128 else 4}> {family} HD {HD} rows {rows} (H {H}) Sk {Sk} {kinds}"
    if rc:
        from kai0_amd._lib import AttnBwdDesc

        a = AttnBwdDesc()
        a.dO, a.O, a.Q, a.K, a.V, a.lse = (t.data_ptr() for t in (dOs, Os, Qs, Ks, Vs, lse))
        a.qcode, a.kcode = (None, None) if d["qcode"] is None else (d["qcode"].data_ptr(), d["kcode"].data_ptr())
        a.P, a.dS, a.dQ = P.data_ptr(), dS.data_ptr(), dQ.data_ptr()
        a.batch, a.rows, a.Sk, a.HD, a.H = B, rows, Sk, HD, H
        a.ldo, a.ldk, a.ldv, a.ldp, a.sO, a.sK, a.sV, a.sP = ld, ld, ld, ldp, dOs.stride(0), Ks.stride(0), Vs.stride(0), P.stride(0)
        a.s_lse = lse.stride(0)
        a.qcode_ld, a.kcode_ld = (0, 0) if d["qcode"] is None else (d["qcode"].stride(0), d["kcode"].stride(0))
        a.scale = d["scale"]
        if expect_refusal:
            assert _lib.load().kai0_attn_bwd_dq2(C.byref(a), stream) != 0, f"{what}: accepted"
            torch.cuda.synchronize()
            for t in (P, dS, dQ):
                assert bool((t == R.SENTINEL).all()), f"{what}: refused, yet wrote an output"
            return
        _lib.call("kai0_attn_bwd_dq2", C.byref(a), stream)
    else:
        _lib.call("kai0_attn_bwd_dq", dOs.data_ptr(), Os.data_ptr(), P.data_ptr(), Ks.data_ptr(), Vs.data_ptr(), dS.data_ptr(), dQ.data_ptr(),
                  B, rows, Sk, HD, ld, ld, ld, ldp, dOs.stride(0), Ks.stride(0), Vs.stride(0), P.stride(0), d["scale"], stream)
    torch.cuda.synchronize()
    note("recompute" if rc else "stored P", what, R.check_bwd(d, P[:, :rows], dS[:, :rows], dQ[:, :rows, :HD], what, rc))
    R.assert_untouched(dS, "dS " + what, rows, ldp)
    R.assert_untouched(dQ, "dQ " + what, rows, HD)
    if rc:
        R.assert_untouched(P, "Pout " + what, rows, ldp)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("rc", (True, False), ids=("recompute", "stored"))
def test_backward_form(ops, rc, family):
    """attn_bwd_dq_kernel<2 | 4, RC>: HD 16 / 72 reach <2, .>, HD 136 / 256 reach <4, .>; recompute through kai0_attn_bwd_dq2 (codes, lse,
    live-tile list), stored P through kai0_attn_bwd_dq.  Sk 129 / 200 / 257 take a second and further trip of the double-buffered loop."""
    for HD, Sq, H, Sk, kinds in R.bwd_cases():
        launch_bwd(ops, family, HD, Sq, H, Sk, kinds, rc)


@pytest.mark.parametrize("kind", R.DEAD_KINDS + (None,))
def test_backward_recompute_dead_tiles(ops, kind):
    """<2, true> and <4, true> with the first / middle / last / every key tile dead (zero-filled P and dS slices, no trip of the loop for
    them) and without codes."""
    for HD in (72, 136):
        for family in ("integer", "peaked"):
            launch_bwd(ops, family, HD, 17, 8, 200, None if kind is None else ("mixed", kind), True)


def test_backward_longest_key_ranges(ops):
    """<2, true> at Sk = 2048, the top of AB_KC_MAX; <2, false> at Sk = 2056; Sk = 2049 is refused by the recompute form with a nonzero
    return and untouched outputs."""
    launch_bwd(ops, "peaked", 16, 24, 1, R.AB_KC_MAX, ("mixed", "dead_mid"), True)
    launch_bwd(ops, "peaked", 16, 24, 1, 2056, ("mixed", "dead_mid"), False)
    launch_bwd(ops, "integer", 16, 24, 1, R.AB_KC_MAX + 1, ("mixed", "dead_mid"), True, expect_refusal=True)


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("batch,Sq", R.DEC_GRIDS)
def test_decode(ops, batch, Sq, family):
    """kai0_attn_decode, HD = 256, H = 8: query tiles x batch = 1 and 32 take dec_logits_kernel<1> + dec_pv_kernel<2>, 33 takes <2> + <4>.
    Both also without codes (Sk 33 and 257: every key below Sk visible, the keys from Sk on hidden by the kernel's own INT_MAX).
    The exact two-pass rounding, so the forward reference with no rescale.  K rows Sk .. k_rows and the transposed cache's columns from
    Sk on hold NaN: the kernel may read them (it does) but nothing of them may reach O."""
    HD, H, q0 = 256, 8, 2
    rows = Sq * H
    for Sk, coded in [(Sk, True) for Sk in R.DEC_SK] + [(Sk, False) for Sk in R.DEC_NO_CODES]:
        q, k, v, scale = (t.to(dev()) if torch.is_tensor(t) else t for t in R.inputs(family, batch, rows, Sk, HD))
        kinds = tuple(R.mask_kinds(Sk)[b % 2] for b in range(batch)) if coded else None  # None: qcode = kcode = NULL
        qcode, kcode = (None if t is None else t.to(dev()) for t in R.codes(kinds, q0 + Sq, Sk))
        vis = R.visible(qcode, kcode, batch, rows, Sk, H, q0, device=dev())
        ref = R.fwd_ref(R.exact_logits(q, k, scale), vis, v, "decode")
        tok = q0 * H + rows + PAD
        Qs = torch.full((batch, tok, HD), R.NAN, dtype=BF16, device=dev())
        Qs[:, q0 * H : q0 * H + rows] = q
        k_rows, vt_ld = Sk + 5, R.round_up(Sk, 32) + PAD
        Ks = torch.full((batch, k_rows, HD + PAD), R.NAN, dtype=BF16, device=dev())
        Ks[:, :Sk, :HD] = k
        Vt = torch.full((batch, HD, vt_ld), R.NAN, dtype=BF16, device=dev())
        Vt[:, :, :Sk] = v.transpose(1, 2)
        O = sentinel(batch, tok, HD)
        ops.attn_decode(Qs, Ks, Vt, O, qcode, kcode, batch=batch, rows=rows, H=H, HD=HD, Sk=Sk, q0=q0, q_bs=tok * HD, k_bs=Ks.stride(0),
                        k_ld=HD + PAD, k_rows=k_rows, vt_bs=Vt.stride(0), vt_ld=vt_ld, scale=scale)
        torch.cuda.synchronize()
        what = f"decode {family} batch {batch} rows {rows} Sk {Sk}{'' if coded else ' no codes'}"
        note("decode", what, R.check_fwd(ref, O[:, q0 * H : q0 * H + rows], None, None, what, Sk))
        O[:, q0 * H : q0 * H + rows] = R.SENTINEL
        assert bool((O == R.SENTINEL).all()), f"{what}: written outside the query rows"
