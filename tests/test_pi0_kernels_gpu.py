"""The HIP entry points pi0's inference stack adds: kai0_linear_f32_rows (the f32 Linears of the per-step suffix embedding, through
ops.pi0_suffix_embed) and kai0_denoise_glue_rows (the step seam over Hs + 1-row samples), against f32 torch on the same inputs."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F32) * scale


def close(got, ref32, mag):
    """tests/pi0_restatement.within_one_bf16_ulp: one bf16 ulp of the reference + the f32 level of a reordered sum (2^-22 x the summed
    magnitudes of the terms, which only matters at the output's zero crossings); -> (all ok, share of bit-equal elements)"""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pi0_restatement as R

    ok, share = R.within_one_bf16_ulp(got, ref32, mag)
    return bool(ok.all()), share


@pytest.mark.parametrize("B,Hs,De,A", [(1, 1, 64, 32), (1, 50, 1024, 32), (2, 50, 1024, 32), (1, 7, 1024, 7)])
def test_pi0_suffix_embed_against_f32_torch(B, Hs, De, A):
    """ops.pi0_suffix_embed == bf16(action_time_mlp_out(silu(action_time_mlp_in(cat[action_in_proj(x_t), time_emb])))) of f32 torch (CPU,
    the reference's single `cat` Linear): every stored bf16 within one bf16 ulp, >= 99 % of them equal (the split of the 2 De
    contraction and the MFMA's k order reorder f32 sums: a rounding may flip); rows 1 .. Hs of every sample written through the row
    map, row 0 and the rows behind the last sample untouched (guard values); the rows' sums of squares to 1e-5.  The last shape has row
    and A tails (M = 7, A = 7)."""
    from kai0_amd import ops

    M, Ss = B * Hs, Hs + 1
    x_t = rnd(M, A, seed=1)
    w_a, b_a = rnd(De, A, seed=2, scale=0.2), rnd(De, seed=3, scale=0.1)
    w_in, b_in = rnd(De, 2 * De, seed=4, scale=De**-0.5), rnd(De, seed=5, scale=0.1)
    w_out, b_out = rnd(De, De, seed=6, scale=2 * De**-0.5), rnd(De, seed=7, scale=0.1)
    te = rnd(De, seed=8)  # the step's time embedding (shared by the batch)
    a = torch.nn.functional.linear(x_t, w_a, b_a)
    cat = torch.cat([a, te[None, :].expand(M, De)], dim=1)
    h = torch.nn.functional.silu(torch.nn.functional.linear(cat, w_in, b_in))
    ref = torch.nn.functional.linear(h, w_out, b_out)
    mag = h.abs() @ w_out.abs().t() + b_out.abs()
    tvec = torch.nn.functional.linear(te[None, :], w_in[:, De:], b_in)[0]  # the hoisted time half (the engine: the library's f32 GEMM)

    d = dev()
    GUARD, extra = 123.0, 3
    xs = torch.full((B * Ss + extra, De), GUARD, dtype=BF16, device=d)
    sq = torch.full((De // 16, B * Ss + extra), -7.0, dtype=F32, device=d)
    ops.pi0_suffix_embed(x_t.to(d), w_a.to(d), b_a.to(d), w_in.to(d), tvec.to(d).contiguous(), w_out.to(d), b_out.to(d), xs, sq, Hs, Ss)
    torch.cuda.synchronize()
    xs_c, sq_c = xs.cpu(), sq.cpu()
    body = xs_c[: B * Ss].view(B, Ss, De)
    assert bool((body[:, 0].float() == GUARD).all()) and bool((xs_c[B * Ss :].float() == GUARD).all()), "row 0 / rows beyond were written"
    got = body[:, 1:].reshape(M, De)
    ok, share = close(got, ref, mag)
    print(f"M={M} De={De} A={A}: within one bf16 ulp: {ok}, bit-equal share {share:.5f}")
    assert ok and share >= 0.99
    rows = (torch.arange(B)[:, None] * Ss + 1 + torch.arange(Hs)[None, :]).reshape(-1)
    state_rows = torch.arange(B) * Ss
    assert bool((sq_c[:, state_rows] == -7.0).all()) and bool((sq_c[:, B * Ss :] == -7.0).all())
    want = got.double().square().sum(1)
    have = sq_c[:, rows].double().sum(0)
    assert float(((have - want).abs() / want).max()) <= 1e-5
    # each partial is its own 16-column tile's
    tile = got.double().square().view(M, De // 16, 16).sum(2).t()
    assert float(((sq_c[:, rows].double() - tile).abs() / (tile + 1e-30)).max()) <= 1e-5


def test_linear_f32_rows_refuses_what_it_cannot_do():
    from kai0_amd import _lib, ops

    d = dev()
    x, w = torch.zeros(4, 64, device=d), torch.zeros(32, 64, device=d)
    out = torch.empty(4, 32, device=d)
    ops.linear_f32_rows(x, w, out_f32=out)
    with pytest.raises(_lib.Kai0HipError):
        ops.linear_f32_rows(torch.zeros(4, 48, device=d), torch.zeros(32, 48, device=d), out_f32=out)  # K % 64
    with pytest.raises(_lib.Kai0HipError):
        ops.linear_f32_rows(torch.zeros(129, 64, device=d), w, out_f32=torch.empty(129, 32, device=d))  # M > 128
    with pytest.raises(ValueError):
        ops.linear_f32_rows(x, w, out_bf16=torch.empty(4, 32, dtype=BF16, device=d), row_map=(2, 3, 1))  # mapped rows past the buffer


@pytest.mark.parametrize("B,Hs", [(1, 50), (2, 50), (2, 7)])
def test_denoise_glue_rows_closes_a_step_over_state_plus_action_rows(B, Hs):
    """The pi0 seam: final plain RMSNorm (as the constant modulation row [w | 0 | 1]) on the LAST Hs of every sample's Hs + 1 rows ->
    action_out_proj -> Euler update, against rmsnorm + linear + Euler in f32 torch (the tolerance of kai0_denoise_glue's test: the dots
    run in another order); at B = 1 the action rows are one contiguous slice and kai0_denoise_glue itself gives the same bits.  And the
    opening half with a row map: the request's state rows bf16(state_proj(state)) into row 0 of every sample, nothing else written."""
    from kai0_amd import ops

    d = dev()
    De, A, Ss, M = 1024, 32, Hs + 1, B * Hs
    xs = (rnd(B * Ss, De, seed=1) * 3).to(BF16)
    w = rnd(De, seed=2, scale=0.2)
    w_out, b_out = rnd(A, De, seed=3, scale=0.05), rnd(A, seed=4, scale=0.1)
    x0 = rnd(M, A, seed=5)
    dt = -0.1
    xa = xs.view(B, Ss, De)[:, 1:].reshape(M, De).float()
    y = (xa * torch.rsqrt(xa.square().mean(-1, keepdim=True) + 1e-6) * (1.0 + w)).to(BF16).float()
    x_ref = x0 + dt * torch.nn.functional.linear(y, w_out, b_out)
    mod = torch.cat([w, torch.zeros(De), torch.ones(De)]).reshape(1, 3 * De).to(d)
    x_t, gxs = x0.to(d), xs.to(d)
    before = gxs.clone()
    ops.denoise_glue(x_t, xs=gxs, mod=mod, mod_ld=3 * De, rows_per_batch=M, eps=1e-6, w_out=w_out.to(d), b_out=b_out.to(d), dt=dt,
                     row_map=(Hs, Ss, 1))
    assert torch.allclose(x_t.cpu(), x_ref, rtol=1e-5, atol=1e-5), float((x_t.cpu() - x_ref).abs().max())
    assert torch.equal(gxs, before)
    if B == 1:
        x_c = x0.to(d)
        ops.denoise_glue(x_c, xs=gxs[1:], mod=mod, mod_ld=3 * De, rows_per_batch=M, eps=1e-6, w_out=w_out.to(d), b_out=b_out.to(d), dt=dt)
        assert torch.equal(x_c, x_t)
    # opening half: state rows
    state = rnd(B, A, seed=6)
    w_s, b_s = rnd(De, A, seed=7, scale=0.2), rnd(De, seed=8, scale=0.1)
    s_ref = torch.nn.functional.linear(state, w_s, b_s)
    buf = torch.full((B * Ss, De), 123.0, dtype=BF16, device=d)
    sq = torch.full((4, B * Ss), -7.0, dtype=F32, device=d)
    st = state.to(d)
    ops.denoise_glue(st, w_in=w_s.to(d), b_in=b_s.to(d), xs_next=buf, rowsq_next=sq, row_map=(1, Ss, 0))
    got = buf.cpu().view(B, Ss, De)
    assert torch.equal(st.cpu(), state) and bool((got[:, 1:].float() == 123.0).all())
    assert close(got[:, 0], s_ref, state.abs() @ w_s.abs().t() + b_s.abs())[0]
    sqc = sq.cpu()
    rows = torch.arange(B) * Ss
    want = got[:, 0].double().square().sum(1)
    assert float(((sqc[0, rows].double() - want).abs() / want).max()) <= 1e-5
    keep = torch.ones(B * Ss, dtype=torch.bool)
    keep[rows] = False
    assert bool((sqc[0, keep] == -7.0).all()) and bool((sqc[1:] == -7.0).all())
