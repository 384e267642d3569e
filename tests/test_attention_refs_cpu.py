"""tests/attention_refs.py held against itself, without a GPU: (a) every f32 emulation (resident, one-pass online, two-pass, decode,
both backward forms, combine) stays inside its float64 bound at every case of the shared tables and for all three input families;
(b) the exact-logit construction does what it says; (c) planted defects — each one a mistake an attention kernel can make at a tile
edge, in the mask or in the online rescale — are rejected by the bounds while the intact emulation passes.

Each test of (a) prints the worst err / bound; the module docstring of attention_refs.py records them."""

import pytest
import torch

import attention_refs as R

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
OUTSIDE = "outside the bound"


def case(family, HD, Sq, H, Sk, q0, kinds):
    B, rows = 2, Sq * H
    q, k, v, scale = R.inputs(family, B, rows, Sk, HD)
    qcode, kcode = R.codes(kinds, q0 + Sq, Sk)
    vis = R.visible(qcode, kcode, B, rows, Sk, H, q0)
    return dict(q=q, k=k, v=v, scale=scale, qcode=qcode, kcode=kcode, vis=vis, s=R.exact_logits(q, k, scale), B=B, rows=rows, Sk=Sk, H=H,
                q0=q0)


def run_fwd(c, kind, ref_kind=None, *, vis=None, defect=None):
    """Emulate `kind` (with vis / defect planted) and hold it against the reference of the intact case."""
    ref = R.fwd_ref(c["s"], c["vis"], c["v"], ref_kind or kind)
    ldp = R.round_up(c["Sk"], 8)
    O, P, lse = R.fwd_emulate(c["s"], c["vis"] if vis is None else vis, c["v"], kind, ldp=ldp, defect=defect)
    return R.check_fwd(ref, O, P, lse, f"{kind} {defect or ''}", c["Sk"])


def merge(worst, w):
    for k, x in w.items():
        worst[k] = max(worst.get(k, 0.0), x)


# ------------------------------------------------------------------------------------------------ (a) emulations inside the bounds
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("form", list(R.FORMS))
def test_forward_emulation_inside_bound(form, family):
    kind = R.FORMS[form][2]
    worst = {}
    for HD, Sq, H, Sk, q0, kinds in R.fwd_cases(form):
        merge(worst, run_fwd(case(family, HD, Sq, H, Sk, q0, kinds), kind))
    print(f"[forward {form} {kind} {family}] worst err / bound " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_decode_emulation_inside_bound(family):
    worst = {}
    for Sk in R.DEC_SK:
        for Sq in (2, 21):
            merge(worst, run_fwd(case(family, 256, Sq, 8, Sk, 0, R.mask_kinds(Sk)), "decode"))
    for Sk in R.DEC_NO_CODES:
        merge(worst, run_fwd(case(family, 256, 21, 8, Sk, 0, None), "decode"))
    print(f"[decode {family}] worst err / bound " + ", ".join(f"{k} {x:.3f}" for k, x in worst.items()))


def bwd_cases():
    """(HD, Sq, H, Sk, kinds, rc): the backward table of tests/test_attention_gpu.py."""
    out = [(*c, rc) for c in R.bwd_cases() for rc in (True, False)]
    for kind in R.DEAD_KINDS:
        out.append((72, 17, 8, 200, ("mixed", kind), True))
    out.append((72, 17, 8, 200, None, True))
    out.append((16, 24, 1, 2048, ("mixed", "dead_mid"), True))
    out.append((16, 24, 1, 2056, ("mixed", "dead_mid"), False))
    return out


def run_bwd(d, rc, defect=None):
    Sk = d["s"].shape[-1]
    Pout, dS, dQ = R.bwd_emulate(d["s"], d["vis"], d["v"], d["k"], d["dO"], d["O"], d["lse"], d["scale"], R.round_up(Sk, 8),
                                 P=None if rc else d["P"], defect=defect)
    return R.check_bwd(d, Pout, dS, dQ, f"{'recompute' if rc else 'stored P'} {defect or ''}", rc)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_backward_emulation_inside_bound(family):
    worst = {True: {}, False: {}}
    for HD, Sq, H, Sk, kinds, rc in bwd_cases():
        merge(worst[rc], run_bwd(R.bwd_inputs(family, 2, Sq * H, Sk, HD, kinds, H), rc))
    for rc, w in worst.items():
        print(f"[backward {'recompute' if rc else 'stored P'} {family}] worst err / bound " + ", ".join(f"{k} {x:.3f}" for k, x in w.items()))


def test_combine_emulation_inside_bound():
    worst = 0.0
    for parts in R.COMBINE_PARTS:
        for HD in R.COMBINE_HD:
            for rows in R.COMBINE_ROWS:
                Op, lse = R.combine_inputs(parts, rows, HD)
                out = R.combine_emulate(Op, lse)
                worst = max(worst, R.assert_within(out, *R.combine_ref(Op, lse), f"combine {parts} x {rows} x {HD}"))
                assert bool((out[torch.isinf(lse).all(0)] == 0).all())
    print(f"[combine] worst err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ (b) the construction
@pytest.mark.parametrize("form", list(R.FORMS))
def test_every_forward_form_meets_every_mask_kind(form):
    """Each forward form's case list holds, at a ragged last tile, a dead first / middle / last tile, all tiles dead, a tile with one
    visible key, the hand-placed codes alone and a case without codes."""
    cases = R.fwd_cases(form)
    kinds = {k for c in cases if c[5] for k in c[5]}
    assert kinds >= set(R.TILE_KINDS) | {"mixed"} and any(c[5] is None for c in cases)
    for kind in R.TILE_KINDS:
        assert any(c[5] and kind in c[5] and c[3] % R.TILE for c in cases), kind
    _, kcode = R.codes(("mixed", "dead_last"), 17, 200)
    assert bool((kcode[1, 192:] == R.INT_MAX).all()) and not bool((kcode[1, :192] == R.INT_MAX).all())


@pytest.mark.parametrize("HD", (16, 72, 136, 256))
def test_ternary_dot_products_are_exact_in_bf16(HD):
    q, k = R.ternary(1, 64, HD, seed=5), R.ternary(1, 300, HD, seed=6)
    k[0, 0] = q[0, 0].abs()  # the extreme: q k = the number of nonzero elements
    q[0, 1], k[0, 1] = 1, -1  # -HD
    n = q.to(F64) @ k.to(F64).transpose(-1, -2)
    assert float(n.min()) == -HD
    assert torch.equal(n.to(F32).to(BF16).to(F64), n)
    assert torch.equal(q.to(F32) @ k.to(F32).transpose(-1, -2), n.to(F32))  # and exact in an f32 summation


def test_count_family_sums_to_the_count():
    for Sk, kinds in ((65, None), (200, ("mixed", "single")), (321, ("mixed", "dead_mid"))):
        c = case("count", 72, 17, 8, Sk, 0, kinds)
        assert bool((c["s"] == 0).all())
        _, _, lse = R.fwd_emulate(c["s"], c["vis"], c["v"], "online")
        count = c["vis"].sum(-1).to(F32)
        assert torch.equal(torch.exp(lse)[count > 0].round(), count[count > 0])
        assert torch.equal(lse, torch.where(count > 0, torch.log(count), torch.full_like(count, R.INF)))


# ------------------------------------------------------------------------------------------------ (c) planted defects
def test_rejects_key_dropped_from_ragged_last_tile():
    c = case("count", 72, 17, 8, 65, 0, None)
    vis = c["vis"].clone()
    vis[..., -1] = False
    for kind in ("online", "twopass", "resident"):
        run_fwd(c, kind)
        with pytest.raises(AssertionError, match=OUTSIDE):
            run_fwd(c, kind, vis=vis)


def test_rejects_key_index_sk_taken_as_visible():
    """Key Sk as the descriptor's zero fill delivers it (k = v = 0): the logit 0 joins the sum."""
    for family in ("count", "integer"):
        c = case(family, 72, 17, 8, 200, 0, None)
        ref = R.fwd_ref(c["s"], c["vis"], c["v"], "online")
        z = torch.zeros(2, 1, 72, dtype=BF16)
        s1 = R.exact_logits(c["q"], torch.cat([c["k"], z], 1), c["scale"])
        O, _, lse = R.fwd_emulate(s1, torch.ones_like(s1, dtype=torch.bool), torch.cat([c["v"], z], 1), "online")
        with pytest.raises(AssertionError, match=OUTSIDE):
            R.check_fwd(ref, O, None, lse, "key Sk visible", 200)


@pytest.mark.parametrize("plant", ("strict", "no_q0", "next_row"))
def test_rejects_mask_defects(plant):
    """< for <=; qcode taken without q0; qcode of row r + 1's position (wrong at every head boundary)."""
    for family in ("count", "integer"):
        c = case(family, 72, 17, 8, 200, 183, ("mixed", "single"))
        kw = {"strict": dict(strict=True), "no_q0": dict(q0=0), "next_row": dict(shift=1)}[plant]
        args = dict(q0=c["q0"])
        args.update(kw)
        vis = R.visible(c["qcode"], c["kcode"], 2, c["rows"], 200, 8, **args)
        for kind in ("online", "twopass"):
            run_fwd(c, kind)
            with pytest.raises(AssertionError, match=OUTSIDE):
                run_fwd(c, kind, vis=vis)


@pytest.mark.parametrize("defect", ("skip_rescale", "lse_last_tile_max"))
def test_rejects_online_softmax_defects(defect):
    """One tile's rescale skipped although the maximum moved; lse built from the last tile's maximum."""
    c = case("peaked", 72, 17, 8, 200, 0, None)
    assert float(R.fwd_ref(c["s"], c["vis"], c["v"], "online")["moves"][0, 0]) == 4  # row 0's maximum moves at every tile
    run_fwd(c, "online")
    with pytest.raises(AssertionError, match=OUTSIDE):
        run_fwd(c, "online", defect=defect)


def test_rejects_single_key_tile_skipped_as_dead():
    for family in R.FAMILIES:
        c = case(family, 72, 17, 8, 200, 0, ("mixed", "single"))
        run_fwd(c, "online")
        with pytest.raises(AssertionError, match=OUTSIDE):
            run_fwd(c, "online", defect="skip_single")


@pytest.mark.parametrize("kind", ("online", "twopass", "resident"))
def test_rejects_p_blocks_exchanged_against_v(kind):
    for family in ("count", "integer"):
        c = case(family, 72, 17, 8, 200, 0, None)
        with pytest.raises(AssertionError, match=OUTSIDE):
            run_fwd(c, kind, defect="swap_p_blocks")


@pytest.mark.parametrize("defect,rc", [("neighbour_D", True), ("neighbour_D", False), ("dq_missing_tile", True), ("dq_missing_tile", False),
                                       ("no_zero_fill", True)])
def test_rejects_backward_defects(defect, rc):
    """dS with the neighbouring row's D; dQ missing one key tile; a dead tile's P / dS slice not zero-filled (the sentinel remains)."""
    d = R.bwd_inputs("integer", 2, 136, 200, 72, ("mixed", "dead_mid"), 8)
    run_bwd(d, rc)
    with pytest.raises(AssertionError, match=OUTSIDE):
        run_bwd(d, rc, defect)


@pytest.mark.parametrize("defect", ("inf_weight_one", "no_max"))
def test_rejects_combine_defects(defect):
    """A part with lse = +inf given weight 1; weights taken without subtracting the maximum at lse ~ 90."""
    Op, lse = R.combine_inputs(3, 33, 72)
    R.assert_within(R.combine_emulate(Op, lse), *R.combine_ref(Op, lse), "combine")
    with pytest.raises(AssertionError, match=OUTSIDE):
        R.assert_within(R.combine_emulate(Op, lse, defect), *R.combine_ref(Op, lse), "combine " + defect)
