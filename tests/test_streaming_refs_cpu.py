"""Calibration of the bounds of tests/streaming_refs.py WITHOUT the kernels: for every operation a plain fp32 torch evaluation with
the header's rounding points (the same formula as the float64 reference, run in float32 and rounded to the stored dtype) is held
against `ulp * |ref| + c * terms + extra` on the inputs the GPU tests use — the hard rows / GELU tails / softmax rows of their
section B and the section A inputs at reduced row counts.  No element may be outside the bound and the worst error / bound must
stay <= 0.5, so a correct fp32 kernel has a factor of two to spare.  Runs on a CPU-only machine."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streaming_refs as R  # noqa: E402
from streaming_refs import BF16, F32, F64  # noqa: E402

NORM_D = [8, 504, 512, 520, 1024, 1536, 2040, 2048]
SOFTMAX_LD = [512, 520, 1024, 1032, 2048, 2056, 4096]
LIMIT = 0.5


def calibrate(fn, stored, *args, c=R.C0, **kw):
    """fn in f64 (reference) and f32 (emulation); `stored`: {output: dtype}.  -> worst ratio over the outputs"""
    ref, emu = fn(*args, dt=F64, **kw), fn(*args, dt=F32, **kw)
    worst = 0.0
    for k, dtype in stored.items():
        r = R.worst_ratio(R.store(emu[k].value, dtype), ref[k], c=c)
        assert r <= LIMIT, f"{fn.__name__}.{k}: fp32 emulation at {r:.3f} of the bound (limit {LIMIT})"
        worst = max(worst, r)
    return worst


def norm_inputs(D, reps=3, seed=0):
    x = R.hard_rows(reps, D, seed=seed)
    return x, R.randn(*x.shape, seed=seed + 1), R.randn(*x.shape, seed=seed + 2)


@pytest.mark.parametrize("D", NORM_D + [64, 1152])
def test_rmsnorm_and_adarms_emulation_within_half_the_bound(D):
    x, dy, dres = norm_inputs(D)
    rows = x.shape[0]
    w = R.randn(D, dtype=F32, seed=5, scale=0.3)
    calibrate(R.rmsnorm_fwd, {"y": BF16, "rstd": F32}, x, w, 1e-6)
    rstd = R.rmsnorm_fwd(x, w, 1e-6, F32)["rstd"].value
    for dr in (None, dres):
        calibrate(R.rmsnorm_bwd, {"dx": BF16, "dw": F32}, dy, x, w, rstd, dr)
    B, rpb = rows // 7, 7
    mod = R.randn(B, 3 * D, dtype=F32, seed=6, scale=0.3)
    calibrate(R.rmsnorm_fwd, {"y": BF16, "rstd": F32}, x, None, 1e-6, mod=mod, rpb=rpb)
    for dg in (None, R.randn(B, D, seed=7)):
        calibrate(R.rmsnorm_bwd, {"dx": BF16, "dmod": F32}, dy, x, None, rstd, dres, mod=mod, rpb=rpb, dgate=dg)


@pytest.mark.parametrize("D", NORM_D + [64, 1152])
def test_layernorm_emulation_within_half_the_bound(D):
    x, dy, dres = norm_inputs(D)
    w = (1 + R.randn(D, seed=5, scale=0.2).float()).to(BF16)
    b = R.randn(D, seed=6, scale=0.2)
    calibrate(R.layernorm_fwd, {"y": BF16, "mean": F32, "rstd": F32}, x, w, b, 1e-6)
    f = R.layernorm_fwd(x, w, b, 1e-6, F32)
    for dr in (None, dres):
        calibrate(R.layernorm_bwd, {"dx": BF16, "dw": BF16, "db": BF16}, dy, x, w, f["mean"].value, f["rstd"].value, dr)


def test_norms_on_plain_inputs_at_reduced_rows():
    """section A's N(0,1) inputs, 700 rows instead of 16 389 / 6147: the column sums see hundreds of addends."""
    for D in (64, 1152):
        x, dy, dres = (R.randn(700, D, seed=s) for s in (1, 2, 3))
        w = R.randn(D, dtype=F32, seed=5, scale=0.3)
        calibrate(R.rmsnorm_fwd, {"y": BF16, "rstd": F32}, x, w, 1e-6)
        rstd = R.rmsnorm_fwd(x, w, 1e-6, F32)["rstd"].value
        calibrate(R.rmsnorm_bwd, {"dx": BF16, "dw": F32}, dy, x, w, rstd, dres)
        wl, bl = (1 + R.randn(D, seed=5, scale=0.2).float()).to(BF16), R.randn(D, seed=6, scale=0.2)
        f = R.layernorm_fwd(x, wl, bl, 1e-6, F32)
        calibrate(R.layernorm_fwd, {"y": BF16, "mean": F32, "rstd": F32}, x, wl, bl, 1e-6)
        calibrate(R.layernorm_bwd, {"dx": BF16, "dw": BF16, "db": BF16}, dy, x, wl, f["mean"].value, f["rstd"].value, dres)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ld", SOFTMAX_LD + [48])
def test_softmax_emulation_within_half_the_bound(ld, masked):
    scores, _, _, allowed = R.softmax_case(ld, masked)
    Sk = ld - 5
    calibrate(R.softmax_fwd, {"probs": BF16}, scores, allowed, Sk)
    ref = R.softmax_fwd(scores, allowed, Sk, F64)["probs"].value
    if masked:
        assert float(ref[:, 4].abs().max()) == 0.0 and float(ref[:, 6, Sk - 3].min()) == 1.0  # the edge rows are what they claim
    # backward on uniform rows (the cancellation case of kai0hip.h) and on the forward's own probabilities
    for probs in (torch.full((37, ld), 1.0 / Sk).to(BF16), ref[0].to(BF16)):
        for dp in (R.randn(37, ld, seed=3), R.randn(37, ld, dtype=F32, seed=4)):
            calibrate(R.softmax_bwd, {"dscores": BF16}, probs, dp, Sk, 0.5)


def test_rowdot_emulation():
    for rows, D in ((300, 256), (99, 8), (99, 72), (99, 512)):
        calibrate(R.rowdot, {"out": F32}, R.randn(rows, D, seed=1), R.randn(rows, D, seed=2))


def test_gelu_family_emulation_on_the_tails():
    n = 16384
    pre = R.gelu_points(n)
    other, third = R.randn(n, seed=1), R.randn(n, seed=2)
    calibrate(R.gelu_fwd, {"y": BF16}, pre)
    calibrate(R.geglu_fwd, {"h": BF16}, pre, other)
    calibrate(R.geglu_bwd, {"du": BF16, "dg": BF16}, third, pre, other)
    calibrate(R.gelu_bwd, {"dx": BF16}, other, pre)
    mixed = R.mix_gelu_points(R.randn(40000, seed=3, scale=3.0))
    calibrate(R.geglu_fwd, {"h": BF16}, mixed, R.randn(40000, seed=4))
    # where the sigmoid saturates the f64 reference is exactly 0 or 1 times the operand: what the GPU tests compare bit for bit
    sat = R.gelu_saturated(pre)
    gp = R.gelu_bwd(torch.ones(n, dtype=BF16), pre, F64)["dx"].value[sat]
    assert int(sat.sum()) == 12 and bool(((gp == 0) | (gp == 1)).all())
    x32 = R.mix_gelu_points(R.randn(40000, seed=5, scale=3.0)).float() * 1.0009765625
    calibrate(R.silu_fwd, {"y": F32}, x32)
    calibrate(R.silu_bwd, {"dx": F32}, R.randn(40000, dtype=F32, seed=6), x32)


def test_gated_embed_colsum_emulation():
    B, rpb, D = 2, 5, 2056
    dout, y, gate = R.randn(B * rpb, D, seed=1), R.randn(B * rpb, D, seed=2), R.randn(B, D, seed=3)
    for dt in (F64, F32):
        dy, res = R.gated_bwd(dout, y, gate, rpb, dt)
    _, ref = R.gated_bwd(dout, y, gate, rpb, F64)
    assert R.worst_ratio(R.store(res["dgate"].value, BF16), ref["dgate"]) <= LIMIT
    assert torch.equal(R.gated_fwd_exact(dout, y, gate, rpb), (dout.float() + (y.float() * gate.float().repeat_interleave(rpb, 0)).to(BF16).float()).to(BF16))
    Bt, T, Dd, V = 3, 200, 136, 50
    tok = R.embed_tokens(Bt, T, V)
    counts = torch.bincount(tok.view(-1), minlength=V)
    assert counts[V - 2] == T and counts[V - 3] == 0 and counts[V - 1] == 0 and 8 <= int(counts[: V - 3].min()) and int(counts[: V - 3].max()) <= 20
    flat = tok.view(-1)
    spread = [int((flat == i).nonzero().max() - (flat == i).nonzero().min()) for i in range(V - 3)]
    assert min(spread) > 256
    do = R.randn(Bt * T, Dd, seed=4)
    ref, occ = R.embed_grad(do, tok, V, 136**0.5, F64)
    emu, _ = R.embed_grad(do, tok, V, 136**0.5, F32)
    assert int(occ.sum()) == V - 2 and R.worst_ratio(R.store(emu.value, BF16), ref) <= LIMIT
    for M, N in ((1, 8), (3, 520), (1023, 8), (4100, 520)):
        calibrate(R.colsum, {"out": BF16}, R.randn(M, N + 16, seed=M), N)
        calibrate(R.colsum, {"out": F32}, R.randn(M, N + 16, seed=M), N)


def test_f32_glue_and_optimizer_emulation():
    n = 50021
    a, b, c3 = (R.randn(n, dtype=F32, seed=s) for s in (1, 2, 3))
    calibrate(R.mse_fwd, {"loss": F32}, a, b)
    calibrate(R.mse_bwd, {"dv": F32}, a, b, c3)
    calibrate(R.euler, {"x": F32}, a, b, -0.1)
    t = torch.rand(7, generator=torch.Generator().manual_seed(0)) * 0.999 + 0.001
    calibrate(R.flow_mix, {"xt": F32, "ut": F32}, a[:49994].view(7, -1), b[:49994].view(7, -1), t)
    master = R.randn(n, seed=4, scale=0.02).float()
    m, v = R.randn(n, dtype=F32, seed=5, scale=1e-2), R.randn(n, dtype=F32, seed=6, scale=1e-2).abs()
    grad, coef = R.randn(n, seed=7), torch.tensor([0.37])
    calibrate(R.adamw, {"master": F32, "m": F32, "v": F32}, master, m, v, grad, coef, 1e-3, 0.9, 0.95, 1e-8, 1e-2, 1 - 0.9**3, 1 - 0.95**3)
    for is_f32, g in ((False, R.randn(200003, seed=8)), (True, R.randn(100003, dtype=F32, seed=9))):
        ref = R.sumsq(g, F64)
        emu = (g.float() ** 2).sum(dtype=F32)  # torch's own blocked f32 sum: a different order, the same class of evaluation
        L = R.sumsq_chain(2**23 if not is_f32 else 2**22, is_f32)
        assert abs(float(emu) - float(ref)) <= LIMIT * (2.0**-23 + L * 2.0**-24) * float(ref)
    assert R.sumsq_chain(2**23 + 8 * 333 + 5, False) == 8 * 2 + 38 and R.sumsq_chain(2**22 + 4 * 333 + 3, True) == 8 * 2 + 38


def test_exact_references_and_builders():
    img = R.randn(2, 3, 28, 28, dtype=F32, seed=1)
    w = R.randn(5, 3, 14, 14, dtype=F32, seed=2)
    cols = R.im2col_ref(img, 14)
    conv = torch.nn.functional.conv2d(img.double(), w.double(), stride=14).flatten(2).transpose(1, 2).reshape(-1, 5)
    assert torch.allclose(cols.double() @ w.double().view(5, -1).t(), conv, atol=1e-9)
    x = R.hard_rows(2, 64)
    assert x.shape == (14, 64) and float(x[0].abs().max()) == 0 and float(x[2].max()) == 100.5 and int((x[2] == 100.5).sum()) == 1
    assert float(x[8].min()) == 100.0 and float(x[8].max()) == 100.0
    pad = torch.tensor([[True, True, False, True]])
    att = torch.tensor([[False, False, False, True]])
    q, k = R.codes_from_pad_att(pad, att)
    assert q.tolist() == [[0, 0, -1, 1]] and k.tolist() == [[0, 0, R.INT_MAX, 1]]
    # a wrong result is seen: one bf16 ulp off in one element of 1e5 is outside the bound, NaN is outside the bound
    a, b = R.randn(100000, seed=1), R.randn(100000, seed=2)
    ref = R.geglu_fwd(a, b, F64)["h"]
    good = R.store(R.geglu_fwd(a, b, F32)["h"].value, BF16)
    assert R.worst_ratio(good, ref) <= LIMIT
    i = int(good.float().abs().argmax())
    for wrong in (good.float()[i] * (1 + 2.0**-5), float("nan")):
        bad = good.clone()
        bad[i] = wrong
        assert R.worst_ratio(bad, ref) == float("inf")
        with pytest.raises(AssertionError, match="1 of 100000"):
            R.assert_within(bad, ref, "probe")
