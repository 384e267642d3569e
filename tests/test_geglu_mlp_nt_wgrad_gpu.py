"""ops.geglu_mlp with its weight gradients on the NT path (both operands K-contiguous: hT, dgT | duT, xT, doutT) against the TN path
(ops.set_mlp_wgrad_nt), forward and backward on one set of inputs:

  * dx is bit-identical between the two paths (the dgrads read the same row-major dg | du);
  * dWg, dWu, dWd of BOTH paths lie inside the per-element f64 bound of tests/gemm_refs.py for the contraction over the rows, against
    an f64 reference built from the same bf16 operands (dout, x, and the h / dg / du the MLP's own act-6 / act-3 launches produce);
  * whether NT and TN agree bit for bit is printed, not required;
  * the NT path is taken where the producers' launches run the 256 x 256 tile, whose epilogues store hT and dgT | duT: F = 2560 at
    rows = 4096 and at rows = 4104 (% 8 == 0, no multiple of a tile: the ragged contraction and ragged producer tiles).  At F = 512
    the producers are 128 x 128 launches and the MLP keeps the TN path — no stand-alone transpose of an [rows][F] operand is made —
    and so does rows = 1600, the action expert's.  Which path ran is read from the launches themselves: ops.gemm is counted per
    layout (plan queries do not pass through ops.gemm), no kernel name is looked at."""

import pytest
import torch

import gemm_refs as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from kai0_amd import ops as _ops

    return _ops


def rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16).to("cuda:0")


def run_mlp(ops, monkeypatch, nt, x, ws, dout):
    """(dx, dWg, dWu, dWd, launches): launches = [(a_kc, b_kc, M, N, K, transposed store?)] of every ops.gemm the MLP made."""
    launches = []
    real = ops.gemm

    def counted(A, B, out, **kw):
        launches.append((kw.get("a_kc", True), kw.get("b_kc", True), kw["M"], kw["N"], kw["K"], kw.get("ct") is not None))
        return real(A, B, out, **kw)

    old = ops.set_mlp_wgrad_nt(nt)
    monkeypatch.setattr(ops, "gemm", counted)
    try:
        xs = x.clone().requires_grad_(True)
        wl = [w.clone().requires_grad_(True) for w in ws]
        ops.geglu_mlp(xs, *wl).backward(dout)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(ops, "gemm", real)
        ops.set_mlp_wgrad_nt(old)
    return xs.grad, wl[0].grad, wl[1].grad, wl[2].grad, launches


@pytest.mark.parametrize("rows,D,F,nt_expected,fused_store", [(4096, 256, 512, False, False), (4104, 256, 512, False, False),
                                                              (4096, 256, 2560, True, True), (4104, 256, 2560, True, True),
                                                              (1600, 256, 512, False, False)])
def test_nt_weight_gradients(ops, monkeypatch, rows, D, F, nt_expected, fused_store):
    x, dout = rnd((rows, D), 1), rnd((rows, D), 2)
    ws = [rnd((F, D), 3, 0.05), rnd((F, D), 4, 0.05), rnd((D, F), 5, 0.05)]
    tn = run_mlp(ops, monkeypatch, False, x, ws, dout)
    nt = run_mlp(ops, monkeypatch, True, x, ws, dout)

    # which path ran: weight gradients are the launches that contract over the rows
    def wgrads(launches):
        return [(a, b) for a, b, M, N, K, _ in launches if K == rows and (M, N) in ((D, F), (F, D), (2 * F, D))]

    assert wgrads(tn[4]) == [(False, False)] * 3, tn[4]
    assert set(wgrads(nt[4])) == ({(True, True)} if nt_expected else {(False, False)}), nt[4]
    assert any(l[5] for l in nt[4]) == fused_store and not any(l[5] for l in tn[4]), nt[4]

    assert torch.equal(tn[0], nt[0]), "dx differs between the NT and the TN path"

    # the operands of the weight gradients, from the MLP's own producer launches (bit for bit what forward and backward made)
    h, g, u = (torch.empty(rows, F, dtype=BF16, device=x.device) for _ in range(3))
    ops.gemm(x, ws[0], h, M=rows, N=F, K=D, lda=D, ldb=D, ldc=F, act=6, B2=ws[1], pre_out=g, pre_out2=u)
    dg, du = torch.empty_like(h), torch.empty_like(h)
    ops.gemm(dout, ops.transpose(ws[2]), dg, M=rows, N=F, K=D, lda=D, ldb=D, ldc=F, act=3, pre_out=du, aux1=g, aux2=u)
    refs = {"dWg": R.reference(dg.t(), x), "dWu": R.reference(du.t(), x), "dWd": R.reference(dout.t(), h)}
    for path, got in (("TN", tn), ("NT", nt)):
        for i, name in enumerate(("dWg", "dWu", "dWd")):
            w = R.assert_within(got[1 + i], *refs[name], f"{name} ({path}, rows {rows})")
            print(f"[rows {rows} F {F}] {name} {path}: worst err / bound {w:.3f}")
    for i, name in enumerate(("dWg", "dWu", "dWd")):
        print(f"[rows {rows} F {F}] {name}: NT and TN bit-identical: {torch.equal(tn[1 + i], nt[1 + i])}")
