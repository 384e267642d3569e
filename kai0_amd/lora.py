"""LoRA adapters on the HIP path: the arithmetic of openpi's `lora.Einsum` / `lora.FeedForward` (src/openpi/models/lora.py:54-65,
:144-148) for nn.Linear-shaped parameters, with its backward.

  y = x W^T + s * bf16( bf16(x A^T) B^T )         A = lora_a.weight [R, in], B = lora_b.weight [out, r], T = bf16(x A^T) [M, R]

every product rounded to bf16 as the reference's bf16 einsums are; `s` = LoRAConfig.scaling_value on the attention projections and
NO scale in the MLP (lora.py:148 ignores alpha).  The delta is added to the pre-activation, before GeGLU / RoPE / a residual gate.

Grouping (`Adapter.heads_up` / `heads_down`, the reference's per-head einsums in the torch layout; N heads, H head_dim, r rank):
  dense            A [r, in],    B [out, r]
  heads_up = N     A [N r, in],  B [N H, r]:    output columns of head n read T[:, n r:(n+1) r] only           (q_proj)
  heads_down = N   A [N r, H],   B [out, N r]:  T[:, n r:(n+1) r] reads input columns n H:(n+1) H only         (o_proj)

Kernels: the products with an activation-sized operand and a rank-sized dimension go to kai0_lora_down / kai0_lora_wgrad
(csrc/lora.hip) where those cover the shape (`lora_down`, `lora_wgrad` below hold the dispatch rule); the rank-r up-projection
(K = r, accumulated into the base GEMM's output: its epilogue rounds bf16(bf16(bf16(acc) * s) + y), the reference's order), the
per-head forms (one batched launch over the heads), the stacked q|k|v down-projection and dx += s dT A are kai0_gemm_bf16
launches.  T is saved for the backward (M x R, small) instead of being recomputed.

The autograd Functions stand beside ops.LinearFn / LinearMultiFn / GegluMlpFn, which models without adapters keep using unchanged.
A base weight gets a gradient only if it requires one (LoRA over an unfrozen base stays correct); adapter gradients are written to
ops._grad_dst, i.e. straight into the sharded trainer's flat gradient buffers.

`merge_lora` folds the adapters into the base weights (serving, export): W + s B A formed in f32 and rounded to bf16 ONCE.  A bf16
merge rounds a small delta into W's ulp (|W| ~ 2^-5 has an ulp of 2^-13; a fresh adapter's delta is ~1e-4 r), which is why training
never merges: the adapters stay separate parameters with f32 masters in the optimizer.

`python -m kai0_amd.lora merge <checkpoint dir or model.safetensors> <out dir>` writes the merged checkpoint of the plain variant.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib, ops
from .ops import BF16, F32, _grad_dst, _grad_ret, _stream, dgrad, gemm, wgrad

DOWN_KERNEL_R = (16, 32, 48, 64)  # kai0_lora_down's R
# The measured dispatch rule (profiles/lora.txt, tools/probes/lora.py): kai0_lora_down beats kai0_gemm_bf16 at K = 1024 / 2048 (1.3-1.7 x),
# does not beat it by more than the interquartile range at M = 30976, K = 16384 (203 vs 225 us) and loses at M = 1600, K = 4096 (25 blocks
# of one K loop each against the GEMM's split-K) — so contractions of 4096 and more go to ops.gemm with ops.pick_split_k's split.
DOWN_KERNEL_MAX_K = 4096
WGRAD_KERNEL_MAX_R = 64  # kai0_lora_wgrad's R (multiples of 8)


class Adapter(NamedTuple):
    """One adapted Linear's pair with its grouping and scale (s = 1.0 in the MLP)."""

    a: torch.Tensor  # lora_a.weight [R, in]
    b: torch.Tensor  # lora_b.weight [out, r]
    scale: float = 1.0
    heads_up: int = 1
    heads_down: int = 1


# ------------------------------------------------------------------------------------------------ raw launches
def lora_down(x, a, out, *, M: int, K: int, R: int, ldx: int, lda: int, ldt: int, x_off: int = 0, a_off: int = 0, t_off: int = 0):
    """out[m][r] = bf16(sum_k x[m][k] a[r][k]) for bf16 buffers with leading dimensions / element offsets (column slices).
    kai0_lora_down where it covers R and is the faster one (K < DOWN_KERNEL_MAX_K), kai0_gemm_bf16 (NT) otherwise."""
    if R in DOWN_KERNEL_R and K % 8 == 0 and K < DOWN_KERNEL_MAX_K:
        _lib.call("kai0_lora_down", x.data_ptr() + 2 * x_off, ldx, a.data_ptr() + 2 * a_off, lda, out.data_ptr() + 2 * t_off, ldt,
                  M, R, K, _stream())  # fmt: skip
    else:
        gemm(x, a, out, M=M, N=R, K=K, lda=ldx, ldb=lda, ldc=ldt, a_off_elems=x_off, b_off_elems=a_off, c_off_elems=t_off,
             split_k=ops.pick_split_k(M, R, K))
    return out


def lora_wgrad(p, q, out, *, M: int, R: int, C: int, ldp: int, ldq: int, ldg: int, scale: float = 1.0, transposed: bool = False,
               p_off: int = 0, q_off: int = 0, g_off: int = 0):  # fmt: skip
    """out = scale * p^T q over the M rows of both: [R][C] at r * ldg + c, or transposed [C][R] at c * ldg + r; out bf16 or f32.
    kai0_lora_wgrad for R <= 64, the TN form of kai0_gemm_bf16 (split over the contraction by its own rule) beyond."""
    if R <= WGRAD_KERNEL_MAX_R and R % 8 == 0 and C % 8 == 0:
        lib = _lib.load()
        nbytes = lib.kai0_lora_wgrad_workspace_bytes(M, R, C)
        ws = ops._workspace(nbytes, p.device)
        esz = out.element_size()
        _lib.call("kai0_lora_wgrad", p.data_ptr() + 2 * p_off, ldp, q.data_ptr() + 2 * q_off, ldq, out.data_ptr() + esz * g_off, ldg,
                  M, R, C, scale, int(transposed), int(out.dtype == F32), ws.data_ptr(), nbytes, _stream())  # fmt: skip
    elif transposed:  # out [C][R] = scale * q^T p
        gemm(q, p, out, M=C, N=R, K=M, a_kc=False, b_kc=False, lda=ldq, ldb=ldp, ldc=ldg, scale=scale, a_off_elems=q_off,
             b_off_elems=p_off, c_off_elems=g_off, split_k=ops.pick_split_k_wgrad(C, R, M))  # fmt: skip
    else:
        gemm(p, q, out, M=R, N=C, K=M, a_kc=False, b_kc=False, lda=ldp, ldb=ldq, ldc=ldg, scale=scale, a_off_elems=p_off,
             b_off_elems=q_off, c_off_elems=g_off, split_k=ops.pick_split_k_wgrad(R, C, M))  # fmt: skip
    return out


def _add_(y, other):
    _lib.call("kai0_add_bf16", y.data_ptr(), other.data_ptr(), y.data_ptr(), y.numel(), _stream())
    return y


def _chk_adapter(ad: Adapter, n_in: int, n_out: int, what: str):
    if ad.a.dtype != BF16 or ad.b.dtype != BF16 or not ad.a.is_contiguous() or not ad.b.is_contiguous():
        raise TypeError(f"{what}: contiguous bf16 adapter weights expected")
    if ad.heads_up > 1 and ad.heads_down > 1:
        raise ValueError(f"{what}: an adapter is grouped on one side only")
    Rt, N = ad.a.shape[0], max(ad.heads_up, ad.heads_down)
    r = Rt // N
    ok = (Rt == N * r and r > 0 and r % 8 == 0 and n_out % (8 * ad.heads_up) == 0 and n_in % (8 * ad.heads_down) == 0
          and tuple(ad.a.shape) == (Rt, n_in // ad.heads_down) and tuple(ad.b.shape) == (n_out, Rt if ad.heads_down > 1 else r))  # fmt: skip
    if not ok:
        raise ValueError(f"{what}: adapter shapes a {tuple(ad.a.shape)} b {tuple(ad.b.shape)} do not fit a [{n_out}, {n_in}] Linear with "
                         f"heads_up={ad.heads_up} heads_down={ad.heads_down} (ranks are multiples of 8)")


# -------------------------------------------------------------------------------- the four products of one adapter
def _down(x, ad: Adapter, T=None, t_off: int = 0, ldt: int | None = None):
    """T = bf16(x A^T) [M, R] (into columns t_off.. of a wider T when given)."""
    M, K = x.shape
    Rt = ad.a.shape[0]
    if T is None:
        T, ldt = torch.empty((M, Rt), dtype=BF16, device=x.device), Rt
    if ad.heads_down == 1:
        lora_down(x, ad.a, T, M=M, K=K, R=Rt, ldx=K, lda=K, ldt=ldt, t_off=t_off)
    else:  # T[:, n r:(n+1) r] = x[:, n H:(n+1) H] A[n r:(n+1) r]^T: one launch, the heads as batch entries
        N = ad.heads_down
        r, H = Rt // N, K // N
        gemm(x, ad.a, T, M=M, N=r, K=H, lda=K, ldb=H, ldc=ldt, batch=N, sA=(H, 0), sB=(r * H, 0), sC=(r, 0), c_off_elems=t_off)
    return T


def _up_acc(T, ad: Adapter, y, t_off: int = 0, ldt: int | None = None):
    """y += s * bf16(T B^T), rounded bf16(bf16(bf16(acc) * s) + y) by the GEMM epilogue."""
    M, n_out = y.shape
    ldt = T.shape[1] if ldt is None else ldt
    r = ad.b.shape[1]
    if ad.heads_up == 1:
        Kt = ad.b.shape[1]  # r, or N r for a head-grouped down-projection
        gemm(T, ad.b, y, M=M, N=n_out, K=Kt, lda=ldt, ldb=Kt, ldc=n_out, scale=ad.scale, accumulate=True, a_off_elems=t_off)
    else:
        N = ad.heads_up
        H = n_out // N
        gemm(T, ad.b, y, M=M, N=H, K=r, lda=ldt, ldb=r, ldc=n_out, batch=N, sA=(r, 0), sB=(H * r, 0), sC=(H, 0), scale=ad.scale,
             accumulate=True, a_off_elems=t_off)  # fmt: skip
    return y


def _dT(dy, ad: Adapter, dT, t_off: int = 0, ldt: int | None = None):
    """dT = bf16(dy B) (unscaled: s is applied where dT is consumed) into columns t_off.. of dT."""
    M, n_out = dy.shape
    ldt = dT.shape[1] if ldt is None else ldt
    Kt = ad.b.shape[1]
    if ad.heads_up > 1:
        N = ad.heads_up
        H = n_out // N
        gemm(dy, ad.b, dT, M=M, N=Kt, K=H, b_kc=False, lda=n_out, ldb=Kt, ldc=ldt, batch=N, sA=(H, 0), sB=(H * Kt, 0), sC=(Kt, 0),
             c_off_elems=t_off)  # fmt: skip
    elif Kt in DOWN_KERNEL_R and n_out % 8 == 0 and n_out < DOWN_KERNEL_MAX_K:
        bt = ops.transpose(ad.b)  # [Kt, out]: tiny
        lora_down(dy, bt, dT, M=M, K=n_out, R=Kt, ldx=n_out, lda=n_out, ldt=ldt, t_off=t_off)
    else:
        gemm(dy, ad.b, dT, M=M, N=Kt, K=n_out, b_kc=False, lda=n_out, ldb=Kt, ldc=ldt, c_off_elems=t_off, split_k=ops.pick_split_k(M, Kt, n_out))
    return dT


def _grad_b(dy, T, ad: Adapter, t_off: int = 0, ldt: int | None = None):
    """d lora_b.weight = s dy^T T."""
    M, n_out = dy.shape
    ldt = T.shape[1] if ldt is None else ldt
    db = _grad_dst(ad.b, BF16)
    Kt = ad.b.shape[1]
    if ad.heads_up > 1:
        N = ad.heads_up
        H = n_out // N
        for n in range(N):
            lora_wgrad(T, dy, db, M=M, R=Kt, C=H, ldp=ldt, ldq=n_out, ldg=Kt, scale=ad.scale, transposed=True, p_off=t_off + n * Kt,
                       q_off=n * H, g_off=n * H * Kt)  # fmt: skip
    else:
        lora_wgrad(T, dy, db, M=M, R=Kt, C=n_out, ldp=ldt, ldq=n_out, ldg=Kt, scale=ad.scale, transposed=True, p_off=t_off)
    return db


def _grad_a(x, dT, ad: Adapter, t_off: int = 0, ldt: int | None = None):
    """d lora_a.weight = s dT^T x."""
    M, K = x.shape
    ldt = dT.shape[1] if ldt is None else ldt
    da = _grad_dst(ad.a, BF16)
    Rt = ad.a.shape[0]
    if ad.heads_down > 1:
        N = ad.heads_down
        r, H = Rt // N, K // N
        for n in range(N):
            lora_wgrad(dT, x, da, M=M, R=r, C=H, ldp=ldt, ldq=K, ldg=H, scale=ad.scale, p_off=t_off + n * r, q_off=n * H, g_off=n * r * H)
    else:
        lora_wgrad(dT, x, da, M=M, R=Rt, C=K, ldp=ldt, ldq=K, ldg=K, scale=ad.scale, p_off=t_off)
    return da


def _dx_acc(dT, ad: Adapter, dx, t_off: int = 0, ldt: int | None = None):
    """dx += s dT A."""
    M, K = dx.shape
    ldt = dT.shape[1] if ldt is None else ldt
    Rt = ad.a.shape[0]
    if ad.heads_down > 1:
        N = ad.heads_down
        r, H = Rt // N, K // N
        gemm(dT, ad.a, dx, M=M, N=H, K=r, b_kc=False, lda=ldt, ldb=H, ldc=K, batch=N, sA=(r, 0), sB=(r * H, 0), sC=(H, 0), scale=ad.scale,
             accumulate=True, a_off_elems=t_off)  # fmt: skip
    else:
        gemm(dT, ad.a, dx, M=M, N=K, K=Rt, b_kc=False, lda=ldt, ldb=K, ldc=K, scale=ad.scale, accumulate=True, a_off_elems=t_off)
    return dx


# -------------------------------------------------------------------------------------------------- autograd
class LoraLinearFn(torch.autograd.Function):
    """y = x W^T + s bf16(bf16(x A^T) B^T) (+ residual, added after the delta): o_proj, and any single adapted Linear."""

    @staticmethod
    def forward(ctx, x, w, a, b, residual, scale: float, heads_up: int, heads_down: int):
        ops._chk(x, BF16, "lora_linear.x")
        ops._chk(w, BF16, "lora_linear.w")
        ad = Adapter(a, b, scale, heads_up, heads_down)
        _chk_adapter(ad, w.shape[1], w.shape[0], "lora_linear")
        y = ops.linear_fwd(x, w)
        T = _down(x, ad)
        _up_acc(T, ad, y)
        if residual is not None:
            _add_(y, residual)
        ctx.save_for_backward(x, w, a, b, T)
        ctx.cfg = (scale, heads_up, heads_down)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dout):
        x, w, a, b, T = ctx.saved_tensors
        ad = Adapter(a, b, *ctx.cfg)
        dy = dout.contiguous()
        need_x, need_w, need_a, need_b = ctx.needs_input_grad[:4]
        dT = None
        if need_x or need_a:
            dT = _dT(dy, ad, torch.empty_like(T))
        dx = None
        if need_x:
            dx = _dx_acc(dT, ad, dgrad(dy, w))
        dw = wgrad(dy, x, w) if need_w else None
        da = _grad_a(x, dT, ad) if need_a else None
        db = _grad_b(dy, T, ad) if need_b else None
        return dx, _grad_ret(w, dw), _grad_ret(a, da), _grad_ret(b, db), (dout if ctx.has_res else None), None, None, None


def lora_linear(x, w, adapter: Adapter, residual=None):
    return LoraLinearFn.apply(x, w, adapter.a, adapter.b, residual, float(adapter.scale), adapter.heads_up, adapter.heads_down)


class LoraLinearMultiFn(torch.autograd.Function):
    """Several adapted Linears of one input (q | k | v): the base projections as ops.LinearMultiFn's stacked GEMM, the adapters'
    down-projections as ONE product over the stacked lora_a weights (T [M, sum R]), then one up-projection per Linear."""

    @staticmethod
    def forward(ctx, x, n: int, cfgs: tuple, *wab):
        ops._chk(x, BF16, "lora_linear_multi.x")
        ws, As, Bs = wab[:n], wab[n : 2 * n], wab[2 * n :]
        ads = [Adapter(a, b, *c) for a, b, c in zip(As, Bs, cfgs)]
        for w, ad in zip(ws, ads):
            _chk_adapter(ad, w.shape[1], w.shape[0], "lora_linear_multi")
            if ad.heads_down > 1:
                raise ValueError("lora_linear_multi: the stacked down-projection is dense")
        M, K = x.shape
        with torch.no_grad():
            outs = ops.linear_multi(x.detach(), [w.detach() for w in ws])
        acat = ops._as_rows([a.detach() for a in As])
        if acat is None:
            acat = torch.cat(As, dim=0)
        Rt = acat.shape[0]
        T = torch.empty((M, Rt), dtype=BF16, device=x.device)
        lora_down(x, acat, T, M=M, K=K, R=Rt, ldx=K, lda=K, ldt=Rt)
        off = 0
        for y, ad in zip(outs, ads):
            _up_acc(T, ad, y, t_off=off, ldt=Rt)
            off += ad.a.shape[0]
        ctx.n, ctx.cfgs = n, cfgs
        ctx.save_for_backward(x, acat, T, *wab)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        n = ctx.n
        x, acat, T, *wab = ctx.saved_tensors
        ws, As, Bs = wab[:n], wab[n : 2 * n], wab[2 * n :]
        ads = [Adapter(a, b, *c) for a, b, c in zip(As, Bs, ctx.cfgs)]
        M, K = x.shape
        Rt = acat.shape[0]
        dev = x.device
        widths = tuple(int(w.shape[0]) for w in ws)
        dys = [torch.zeros((M, wd), dtype=BF16, device=dev) if d is None else d for d, wd in zip(douts, widths)]
        need = ctx.needs_input_grad
        need_x, need_w, need_a, need_b = need[0], need[3 : 3 + n], need[3 + n : 3 + 2 * n], need[3 + 2 * n :]
        dT = torch.empty((M, Rt), dtype=BF16, device=dev)
        off = 0
        for dy, ad in zip(dys, ads):
            _dT(dy if dy.is_contiguous() else dy.contiguous(), ad, dT, t_off=off, ldt=Rt)
            off += ad.a.shape[0]
        dx = None
        if need_x:
            dycat = ops._as_fused(dys, widths)
            wcat = ops._as_rows([w.detach() for w in ws])
            if dycat is not None or wcat is not None:  # one dgrad over the stacked projection
                dycat = torch.cat(dys, dim=1) if dycat is None else dycat
                dx = dgrad(dycat, torch.cat(ws, dim=0) if wcat is None else wcat)
            else:
                for i, (dy, w) in enumerate(zip(dys, ws)):
                    dx = dgrad(dy.contiguous(), w, dx, accumulate=i > 0, split=i == 0)  # (the accumulating ones unsplit: as found)
            scales = {ad.scale for ad in ads}
            if len(scales) == 1:  # dx += s dT Acat: one launch over the stacked adapters
                _dx_acc(dT, Adapter(acat, acat, scales.pop()), dx)
            else:
                off = 0
                for ad in ads:
                    _dx_acc(dT, ad, dx, t_off=off, ldt=Rt)
                    off += ad.a.shape[0]
        dws, das, dbs = [None] * n, [None] * n, [None] * n
        off = 0
        for i, (dy, w, ad) in enumerate(zip(dys, ws, ads)):
            dyc = dy if dy.is_contiguous() else dy.contiguous()
            if need_w[i]:
                dws[i] = _grad_ret(w, wgrad(dyc, x, w))
            if need_a[i]:
                das[i] = _grad_ret(ad.a, _grad_a(x, dT, ad, t_off=off, ldt=Rt))
            if need_b[i]:
                dbs[i] = _grad_ret(ad.b, _grad_b(dyc, T, ad, t_off=off, ldt=Rt))
            off += ad.a.shape[0]
        return (dx, None, None, *dws, *das, *dbs)


def lora_linear_multi(x, weights, adapters):
    n = len(weights)
    cfgs = tuple((float(ad.scale), ad.heads_up, ad.heads_down) for ad in adapters)
    return LoraLinearMultiFn.apply(x, n, cfgs, *weights, *[ad.a for ad in adapters], *[ad.b for ad in adapters])


class LoraGegluMlpFn(torch.autograd.Function):
    """Gemma MLP with adapters on gate_proj, up_proj and down_proj (lora.py:123-148; no scale).  The deltas enter g and u BEFORE
    GeGLU, so the fused gate | up GEMM of ops.GegluMlpFn (which applies GeGLU in registers) cannot be used: g and u are plain GEMMs,
    the stacked gate | up down-projection is one kai0_lora_down (R = 2 r), and GeGLU is the element-wise kernel — one extra pass over
    g, u and h per layer.  Backward: dh = dout Wd + dTd Ad is ONE GEMM over the concatenated contraction ([dout | dTd] against
    [Wd^T | Ad^T]) so that the GeGLU-backward epilogue (act 3, on the post-adapter g and u) still sees the whole dh."""

    @staticmethod
    def forward(ctx, x, wg, wu, wd, ag, bg, au, bu, ad_, bd, residual):
        ops._chk(x, BF16, "lora_geglu_mlp.x")
        M, D = x.shape
        F = wg.shape[0]
        Ag, Au, Ad = Adapter(ag, bg), Adapter(au, bu), Adapter(ad_, bd)
        _chk_adapter(Ag, D, F, "lora_geglu_mlp.gate")
        _chk_adapter(Au, D, F, "lora_geglu_mlp.up")
        _chk_adapter(Ad, F, D, "lora_geglu_mlp.down")
        r = ag.shape[0]
        if au.shape[0] != r:
            raise ValueError("lora_geglu_mlp: gate and up adapters of one rank expected")
        g = ops.linear_fwd(x, wg)
        u = ops.linear_fwd(x, wu)
        agu = ops._as_rows([ag.detach(), au.detach()])
        if agu is None:
            agu = torch.cat([ag, au], dim=0)
        Tgu = torch.empty((M, 2 * r), dtype=BF16, device=x.device)
        lora_down(x, agu, Tgu, M=M, K=D, R=2 * r, ldx=D, lda=D, ldt=2 * r)
        _up_acc(Tgu, Ag, g, t_off=0, ldt=2 * r)
        _up_acc(Tgu, Au, u, t_off=r, ldt=2 * r)
        h = ops.geglu_fwd(g, u)
        y = ops.linear_fwd(h, wd)
        Td = _down(h, Ad)
        _up_acc(Td, Ad, y)
        if residual is not None:
            _add_(y, residual)
        ctx.save_for_backward(x, wg, wu, wd, ag, bg, au, bu, ad_, bd, agu, g, u, h, Tgu, Td)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dout):
        x, wg, wu, wd, ag, bg, au, bu, ad_, bd, agu, g, u, h, Tgu, Td = ctx.saved_tensors
        Ag, Au, Ad = Adapter(ag, bg), Adapter(au, bu), Adapter(ad_, bd)
        dout = dout.contiguous()
        M, D = x.shape
        F = wg.shape[0]
        r = ag.shape[0]
        dev = x.device
        need = ctx.needs_input_grad
        dwd = wgrad(dout, h, wd) if need[3] else None
        dbd = _grad_b(dout, Td, Ad) if need[9] else None
        # [dout | dTd] [M, D + r] and [Wd^T | Ad^T] [F, D + r]: dh = dout Wd + dTd Ad in one contraction
        Kc = D + r
        lhs = torch.empty((M, Kc), dtype=BF16, device=dev)
        lhs[:, :D].copy_(dout)
        _dT(dout, Ad, lhs, t_off=D, ldt=Kc)
        rhs = torch.empty((F, Kc), dtype=BF16, device=dev)
        ops.transpose_strided(wd, rhs, R=D, C=F, src_ld=F, dst_ld=Kc)
        ops.transpose_strided(ad_, rhs[:, D:], R=r, C=F, src_ld=F, dst_ld=Kc)
        dad = _grad_a(h, lhs, Ad, t_off=D, ldt=Kc) if need[8] else None
        dg = torch.empty((M, F), dtype=BF16, device=dev)
        du = torch.empty((M, F), dtype=BF16, device=dev)
        gemm(lhs, rhs, dg, M=M, N=F, K=Kc, lda=Kc, ldb=Kc, ldc=F, act=3, pre_out=du, aux1=g, aux2=u)
        del lhs, rhs
        dwg = wgrad(dg, x, wg) if need[1] else None
        dwu = wgrad(du, x, wu) if need[2] else None
        dbg = _grad_b(dg, Tgu, Ag, t_off=0, ldt=2 * r) if need[5] else None
        dbu = _grad_b(du, Tgu, Au, t_off=r, ldt=2 * r) if need[7] else None
        dag = dau = dx = None
        if need[0] or need[4] or need[6]:
            dTgu = torch.empty((M, 2 * r), dtype=BF16, device=dev)
            _dT(dg, Ag, dTgu, t_off=0, ldt=2 * r)
            _dT(du, Au, dTgu, t_off=r, ldt=2 * r)
            if need[4] or need[6]:
                dsts = [_grad_dst(ag, BF16), _grad_dst(au, BF16)]
                dagu = ops._as_rows(dsts)
                tmp = dagu is None
                if tmp:
                    dagu = torch.empty((2 * r, D), dtype=BF16, device=dev)
                lora_wgrad(dTgu, x, dagu, M=M, R=2 * r, C=D, ldp=2 * r, ldq=D, ldg=D)
                if tmp:
                    dsts[0].copy_(dagu[:r])
                    dsts[1].copy_(dagu[r:])
                dag, dau = (dsts[0] if need[4] else None), (dsts[1] if need[6] else None)
            if need[0]:
                dx = dgrad(du, wu, dgrad(dg, wg), accumulate=True, split=False)  # (the accumulating one unsplit: as found)
                _dx_acc(dTgu, Adapter(agu, agu), dx)
        return (dx, _grad_ret(wg, dwg), _grad_ret(wu, dwu), _grad_ret(wd, dwd), _grad_ret(ag, dag), _grad_ret(bg, dbg),
                _grad_ret(au, dau), _grad_ret(bu, dbu), _grad_ret(ad_, dad), _grad_ret(bd, dbd), (dout if ctx.has_res else None))  # fmt: skip


def lora_geglu_mlp(x, wg, wu, wd, gate: Adapter, up: Adapter, down: Adapter, residual=None):
    for ad in (gate, up, down):
        if ad.scale != 1.0 or ad.heads_up != 1 or ad.heads_down != 1:
            raise ValueError("lora_geglu_mlp: the MLP adapters are dense and unscaled (lora.py:144-148 ignores alpha)")
    return LoraGegluMlpFn.apply(x, wg, wu, wd, gate.a, gate.b, up.a, up.b, down.a, down.b, residual)


# ------------------------------------------------------------------------------------------- merging (serving, export)
def adapter_delta(a, b, scale: float = 1.0, heads_up: int = 1, heads_down: int = 1, dtype=F32):
    """s B A as a dense [out, in] matrix in `dtype`, respecting the per-head structure."""
    a, b = a.to(dtype), b.to(dtype)
    if heads_up > 1:
        N, r = heads_up, b.shape[1]
        d = torch.einsum("nhr,nri->nhi", b.view(N, -1, r), a.view(N, r, -1)).reshape(b.shape[0], a.shape[1])
    elif heads_down > 1:
        N, H = heads_down, a.shape[1]
        d = torch.einsum("onr,nrh->onh", b.view(b.shape[0], N, -1), a.view(N, -1, H)).reshape(b.shape[0], N * H)
    else:
        d = b @ a
    return d * scale


def merged_weight(w, a, b, scale: float = 1.0, heads_up: int = 1, heads_down: int = 1):
    """W + s B A formed in f32 and rounded to W's dtype once."""
    return (w.to(F32) + adapter_delta(a, b, scale, heads_up, heads_down)).to(w.dtype)


def plain_variant(variant: str) -> str:
    return variant[: -len("_lora")] if variant.endswith("_lora") else variant


def _name_spec(name: str, model_config):
    """(scale, heads_up, heads_down) of the adapted Linear whose state-dict prefix is `name` (ending in `q_proj.` etc.)."""
    from .config import get_config

    cfg = get_config(model_config.action_expert_variant if ".gemma_expert." in name else model_config.paligemma_variant)
    leaf = name.rstrip(".").rsplit(".", 1)[-1]
    if leaf in ("gate_proj", "up_proj", "down_proj"):
        return 1.0, 1, 1
    s = cfg.lora_configs["attn"].scaling_value
    return {"q_proj": (s, cfg.num_heads, 1), "k_proj": (s, 1, 1), "v_proj": (s, 1, 1), "o_proj": (s, 1, cfg.num_heads)}[leaf]


def merge_lora(state_dict: dict, model_config) -> dict:
    """The state dict of the plain variant (`plain_variant`) computing what the LoRA model computes up to one bf16 rounding per
    weight: every `<linear>.lora_a.weight` / `.lora_b.weight` pair is folded into `<linear>.weight` (module docstring: why a bf16
    merge is for serving and export only)."""
    out = {k: v for k, v in state_dict.items() if ".lora_" not in k}
    for k, a in state_dict.items():
        if not k.endswith(".lora_a.weight"):
            continue
        pre = k[: -len("lora_a.weight")]
        out[pre + "weight"] = merged_weight(state_dict[pre + "weight"], a, state_dict[pre + "lora_b.weight"], *_name_spec(pre, model_config))
    return out


class _Overlay:
    """`base` with some attributes replaced (everything else is read through)."""

    def __init__(self, base, **over):
        self.__dict__["_base"] = base
        self.__dict__.update(over)

    def __getattr__(self, name):
        return getattr(self.__dict__["_base"], name)


def has_adapters(module) -> bool:
    return any(getattr(m, "lora", None) is not None for m in module.modules())


def merged_view(pe):
    """A read-only stand-in for a PaliGemmaWithExpertModel whose adapted Gemma Linears present `weight` = W + s B A (fresh copies: the
    inference engine's, like its stacked ones) and no adapters; every other module is the original."""

    def lin(mod):
        if getattr(mod, "lora", None) is None:
            return mod
        with torch.no_grad():
            w = merged_weight(mod.weight, mod.lora_a.weight, mod.lora_b.weight, *mod.lora)
        return _Overlay(mod, weight=w, lora=None)

    def tower(gm):
        layers = []
        for l in gm.layers:
            at, mlp = l.self_attn, l.mlp
            layers.append(_Overlay(l, self_attn=_Overlay(at, q_proj=lin(at.q_proj), k_proj=lin(at.k_proj), v_proj=lin(at.v_proj), o_proj=lin(at.o_proj)),
                                   mlp=_Overlay(mlp, gate_proj=lin(mlp.gate_proj), up_proj=lin(mlp.up_proj), down_proj=lin(mlp.down_proj))))  # fmt: skip
        return _Overlay(gm, layers=layers)

    pg = pe.paligemma
    lm = tower(pg.model.language_model)
    return _Overlay(pe, paligemma=_Overlay(pg, model=_Overlay(pg.model, language_model=lm), language_model=lm),
                    gemma_expert=_Overlay(pe.gemma_expert, model=tower(pe.gemma_expert.model)))  # fmt: skip


def _main(argv):
    import argparse
    import os

    import safetensors.torch

    from .config import Pi0Config

    ap = argparse.ArgumentParser(prog="python -m kai0_amd.lora")
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="fold the adapters of a LoRA checkpoint into its base weights")
    m.add_argument("checkpoint", help="a checkpoint directory or its model.safetensors")
    m.add_argument("out", help="directory that receives model.safetensors of the plain variant")
    m.add_argument("--paligemma-variant", default="gemma_2b_lora")
    m.add_argument("--action-expert-variant", default="gemma_300m_lora")
    args = ap.parse_args(argv)
    path = os.path.join(args.checkpoint, "model.safetensors") if os.path.isdir(args.checkpoint) else args.checkpoint
    sd = safetensors.torch.load_file(path)
    cfg = Pi0Config(paligemma_variant=args.paligemma_variant, action_expert_variant=args.action_expert_variant)
    merged = merge_lora(sd, cfg)
    os.makedirs(args.out, exist_ok=True)
    with safetensors.safe_open(path, "pt") as f:
        meta = f.metadata()  # the tied-weight aliases travel with the file
    safetensors.torch.save_file({k: v.contiguous() for k, v in merged.items()}, os.path.join(args.out, "model.safetensors"), metadata=meta)
    print(f"merged {sum(k.endswith('.lora_a.weight') for k in sd)} adapters ({plain_variant(cfg.paligemma_variant)} / "
          f"{plain_variant(cfg.action_expert_variant)}) into {args.out}")


if __name__ == "__main__":
    import sys

    _main(sys.argv[1:])
