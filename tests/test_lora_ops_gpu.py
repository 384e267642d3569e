"""kai0_amd.lora's autograd Functions (lora_linear: dense, per-head up as q_proj, per-head down as o_proj, with and without a
residual; lora_linear_multi; lora_geglu_mlp) against an fp32 torch restatement of the adapter arithmetic on the same bf16 values
(openpi lora.py:54-65 `Einsum`: result + (x A) B * s; :144-148 `FeedForward._dot`: no s), at the shapes and tolerances of
tests/test_kernels_gpu.py's test_linear_autograd / test_geglu_mlp_fused (M = 264 / 300, widths 136 .. 328; forward rel-L2 < 6e-3,
every gradient < 1.5e-2).  Ranks 16 (kai0_lora_down / kai0_lora_wgrad) and 8 (the project's test variant: partly the GEMM
dispatch); the adapter weights are drawn large enough (0.1) that the delta is a sizeable share of the output."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FWD_TOL, GRAD_TOL = 6e-3, 1.5e-2


@pytest.fixture(scope="module")
def L():
    from kai0_amd import lora

    return lora


def rnd(*shape, seed=0, scale=1.0, grad=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = (torch.randn(*shape, generator=g) * scale).to(BF16).to("cuda:0")
    return t.requires_grad_(True) if grad else t


def rel_err(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def ref_delta(x, a, b, s, heads_up=1, heads_down=1):
    """fp32: s * (x A^T) B^T in the grouped torch layout (the table of kai0_amd/lora.py)."""
    M = x.shape[0]
    if heads_up > 1:
        N, r = heads_up, b.shape[1]
        T = (x @ a.t()).view(M, N, r)
        return torch.einsum("mnr,nhr->mnh", T, b.view(N, -1, r)).reshape(M, -1) * s
    if heads_down > 1:
        N, H = heads_down, a.shape[1]
        T = torch.einsum("mnh,nrh->mnr", x.view(M, N, H), a.view(N, -1, H)).reshape(M, -1)
        return (T @ b.t()) * s
    return ((x @ a.t()) @ b.t()) * s


def f32_leaves(*ts):
    return [t.detach().float().requires_grad_(True) for t in ts]


def check_grads(names, ts, refs):
    for n, t, r in zip(names, ts, refs):
        assert t.grad is not None, f"{n}: no gradient"
        e = rel_err(t.grad, r.grad)
        print(f"{n}: {e:.3e}")
        assert e < GRAD_TOL, f"{n}: {e:.3e}"


LINEAR_CASES = {  # name: (in, out, a shape, b shape, heads_up, heads_down)
    "dense_r16": (200, 328, (16, 200), (328, 16), 1, 1),
    "dense_r8": (200, 328, (8, 200), (328, 8), 1, 1),
    "q_r16": (200, 256, (64, 200), (256, 16), 4, 1),
    "q_r8": (200, 256, (32, 200), (256, 8), 4, 1),
    "o_r16": (256, 200, (64, 64), (200, 64), 1, 4),
    "o_r8": (256, 200, (32, 64), (200, 32), 1, 4),
}


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("case", list(LINEAR_CASES))
def test_lora_linear(L, case, residual):
    n_in, n_out, sa, sb, hu, hd = LINEAR_CASES[case]
    M, s = 264, 2.0
    x, w = rnd(M, n_in, seed=1, grad=True), rnd(n_out, n_in, seed=2, scale=0.08, grad=True)
    a, b = rnd(*sa, seed=3, scale=0.1, grad=True), rnd(*sb, seed=4, scale=0.1, grad=True)
    res = rnd(M, n_out, seed=5, grad=True) if residual else None
    dy = rnd(M, n_out, seed=6)
    out = L.lora_linear(x, w, L.Adapter(a, b, s, hu, hd), res)
    out.backward(dy)
    xr, wr, ar, br = f32_leaves(x, w, a, b)
    ref = xr @ wr.t() + ref_delta(xr, ar, br, s, hu, hd)
    if residual:
        ref = ref + res.detach().float()
    ref.backward(dy.float())
    share = float(ref_delta(xr, ar, br, s, hu, hd).detach().norm() / ref.detach().norm())
    assert share > 0.05, f"the adapter's share of the output is {share:.3f}: the test would not see it"
    e = rel_err(out, ref)
    print(f"{case} residual={residual}: forward {e:.3e}, adapter share {share:.2f}")
    assert e < FWD_TOL
    check_grads(("dx", "dw", "dA", "dB"), (x, w, a, b), (xr, wr, ar, br))
    if residual:
        assert torch.equal(res.grad, dy)


def test_lora_linear_frozen_base_gets_no_gradient(L):
    M = 264
    x, w = rnd(M, 200, seed=1, grad=True), rnd(328, 200, seed=2, scale=0.08)
    a, b = rnd(16, 200, seed=3, scale=0.1, grad=True), rnd(328, 16, seed=4, scale=0.1, grad=True)
    dy = rnd(M, 328, seed=6)
    L.lora_linear(x, w, L.Adapter(a, b, 2.0)).backward(dy)
    assert w.grad is None
    xr, ar, br = f32_leaves(x, a, b)
    (xr @ w.float().t() + ref_delta(xr, ar, br, 2.0)).backward(dy.float())
    check_grads(("dx", "dA", "dB"), (x, a, b), (xr, ar, br))


def test_zero_b_equals_the_plain_ops_bit_for_bit(L):
    from kai0_amd import ops

    M = 264
    x, w, res = rnd(M, 200, seed=1), rnd(328, 200, seed=2, scale=0.08), rnd(M, 328, seed=5)
    a, b0 = rnd(16, 200, seed=3, scale=0.1), torch.zeros(328, 16, dtype=BF16, device="cuda:0")
    assert torch.equal(L.lora_linear(x, w, L.Adapter(a, b0, 2.0), res), ops.linear(x, w, None, res))
    assert torch.equal(L.lora_linear(x, w, L.Adapter(a, b0, 2.0)), ops.linear(x, w))
    wq, wk, wv = rnd(256, 200, seed=7, scale=0.08), rnd(136, 200, seed=8, scale=0.08), rnd(136, 200, seed=9, scale=0.08)
    ads = [L.Adapter(rnd(64, 200, seed=10, scale=0.1), torch.zeros(256, 16, dtype=BF16, device="cuda:0"), 2.0, 4, 1),
           L.Adapter(rnd(16, 200, seed=11, scale=0.1), torch.zeros(136, 16, dtype=BF16, device="cuda:0"), 2.0),
           L.Adapter(rnd(16, 200, seed=12, scale=0.1), torch.zeros(136, 16, dtype=BF16, device="cuda:0"), 2.0)]  # fmt: skip
    for got, want in zip(L.lora_linear_multi(x, [wq, wk, wv], ads), ops.linear_multi(x, [wq, wk, wv])):
        assert torch.equal(got, want)
    for Fd in (328, 128):  # the two-GEMM and the pair-GEMM form of ops.geglu_mlp
        xm, wg, wu, wd = rnd(300, 136, seed=1), rnd(Fd, 136, seed=2, scale=0.1), rnd(Fd, 136, seed=3, scale=0.1), rnd(136, Fd, seed=4, scale=0.1)
        rm = rnd(300, 136, seed=5)
        zero = lambda n_out: torch.zeros(n_out, 16, dtype=BF16, device="cuda:0")  # noqa: E731
        got = L.lora_geglu_mlp(xm, wg, wu, wd, L.Adapter(rnd(16, 136, seed=6), zero(Fd)), L.Adapter(rnd(16, 136, seed=7), zero(Fd)),
                               L.Adapter(rnd(16, Fd, seed=8), zero(136)), rm)  # fmt: skip
        assert torch.equal(got, ops.geglu_mlp(xm, wg, wu, wd, rm)), f"F = {Fd}"


@pytest.mark.parametrize("r", [16, 8])
@pytest.mark.parametrize("base_grad", [True, False])
def test_lora_linear_multi(L, r, base_grad):
    M, D, N, H, s = 264, 200, 4, 64, 2.0
    x = rnd(M, D, seed=1, grad=True)
    ws = [rnd(n, D, seed=2 + i, scale=0.08, grad=base_grad) for i, n in enumerate((N * H, 136, 136))]
    As = [rnd(n, D, seed=5 + i, scale=0.1, grad=True) for i, n in enumerate((N * r, r, r))]
    Bs = [rnd(n, r, seed=8 + i, scale=0.1, grad=True) for i, n in enumerate((N * H, 136, 136))]
    hus = (N, 1, 1)
    dys = [rnd(M, n, seed=11 + i) for i, n in enumerate((N * H, 136, 136))]
    outs = L.lora_linear_multi(x, ws, [L.Adapter(a, b, s, hu, 1) for a, b, hu in zip(As, Bs, hus)])
    torch.autograd.backward(outs, dys)
    xr, *rest = f32_leaves(x, *ws, *As, *Bs)
    wr, ar, br = rest[:3], rest[3:6], rest[6:]
    refs = [xr @ w.t() + ref_delta(xr, a, b, s, hu) for w, a, b, hu in zip(wr, ar, br, hus)]
    torch.autograd.backward(refs, [d.float() for d in dys])
    for name, o, rf in zip("qkv", outs, refs):
        e = rel_err(o, rf)
        print(f"{name}: forward {e:.3e}")
        assert e < FWD_TOL
    check_grads(["dx"] + [f"dA_{n}" for n in "qkv"] + [f"dB_{n}" for n in "qkv"], [x, *As, *Bs], [xr, *ar, *br])
    if base_grad:
        check_grads([f"dw_{n}" for n in "qkv"], ws, wr)
    else:
        assert all(w.grad is None for w in ws)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("base_grad", [True, False])
@pytest.mark.parametrize("M,D,Fd,r", [(300, 136, 328, 16), (264, 200, 136, 8), (300, 64, 128, 16)])
def test_lora_geglu_mlp(L, M, D, Fd, r, base_grad, residual):
    x = rnd(M, D, seed=1, grad=True)
    wg, wu = (rnd(Fd, D, seed=s, scale=0.1, grad=base_grad) for s in (2, 3))
    wd = rnd(D, Fd, seed=4, scale=0.1, grad=base_grad)
    ag, au, ad = rnd(r, D, seed=5, scale=0.1, grad=True), rnd(r, D, seed=6, scale=0.1, grad=True), rnd(r, Fd, seed=7, scale=0.1, grad=True)
    bg, bu, bd = rnd(Fd, r, seed=8, scale=0.1, grad=True), rnd(Fd, r, seed=9, scale=0.1, grad=True), rnd(D, r, seed=10, scale=0.1, grad=True)
    res = rnd(M, D, seed=11, grad=True) if residual else None
    dy = rnd(M, D, seed=12)
    out = L.lora_geglu_mlp(x, wg, wu, wd, L.Adapter(ag, bg), L.Adapter(au, bu), L.Adapter(ad, bd), res)
    out.backward(dy)
    leaves = (x, wg, wu, wd, ag, bg, au, bu, ad, bd)
    xr, gr, ur, dr, agr, bgr, aur, bur, adr, bdr = refs = f32_leaves(*leaves)
    g = xr @ gr.t() + ref_delta(xr, agr, bgr, 1.0)
    u = xr @ ur.t() + ref_delta(xr, aur, bur, 1.0)
    h = torch.nn.functional.gelu(g, approximate="tanh") * u
    ref = h @ dr.t() + ref_delta(h, adr, bdr, 1.0)
    if residual:
        ref = ref + res.detach().float()
    ref.backward(dy.float())
    e = rel_err(out, ref)
    print(f"mlp {M}x{D}x{Fd} r{r}: forward {e:.3e}")
    assert e < FWD_TOL
    names = ("dx", "dwg", "dwu", "dwd", "dA_gate", "dB_gate", "dA_up", "dB_up", "dA_down", "dB_down")
    keep = [i for i in range(10) if base_grad or i not in (1, 2, 3)]
    check_grads([names[i] for i in keep], [leaves[i] for i in keep], [refs[i] for i in keep])
    if not base_grad:
        assert wg.grad is None and wu.grad is None and wd.grad is None
    if residual:
        assert torch.equal(res.grad, dy)


def test_lora_geglu_mlp_rejects_a_scale(L):
    x, wg, wu, wd = rnd(64, 64), rnd(128, 64), rnd(128, 64), rnd(64, 128)
    a1, b1, a2, b2 = rnd(8, 64), rnd(128, 8), rnd(8, 128), rnd(64, 8)
    with pytest.raises(ValueError):
        L.lora_geglu_mlp(x, wg, wu, wd, L.Adapter(a1, b1, 2.0), L.Adapter(a1, b1), L.Adapter(a2, b2))
