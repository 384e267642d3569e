"""Fused AdamW + global-norm clipping on the HIP kernels, and the reference's LR schedule.

Semantics follow scripts/train_pytorch.py:469-491,557-561 (torch.optim.AdamW + clip_grad_norm_) and
src/openpi/training/optimizer.py:15-85 (warmup + cosine).  Difference, on purpose and documented in DESIGN.md:
the reference's PyTorch trainer updates bf16 parameters in bf16 with bf16 Adam moments; here every parameter has
an f32 master copy and f32 moments (the JAX trainer's precision), and the bf16 model copy is re-rounded from the
master each step.  16 B/param of optimizer state is HBM-bound work, fused into one pass per tensor.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .ops import BF16, F32, _stream


def lr_schedule(step: int, *, warmup_steps: int, peak_lr: float, decay_steps: int, end_lr: float) -> float:
    """train_pytorch.py:483-491 (matches optax warmup_cosine_decay_schedule with init = peak/(warmup+1))."""
    if step < warmup_steps:
        init_lr = peak_lr / (warmup_steps + 1)
        return init_lr + (peak_lr - init_lr) * step / warmup_steps
    progress = min(1.0, (step - warmup_steps) / max(1, decay_steps - warmup_steps))
    cos = 0.5 * (1 + np.cos(np.pi * progress))
    return float(end_lr + (peak_lr - end_lr) * cos)


WEIGHT_UPDATES = [0]  # bumped by every parameter update made through the HIP kernels (see infer.InferenceEngine._fingerprint)


def adamw_step_(master, m, v, grad, param, *, lr, beta1, beta2, eps, wd, step: int, clip_coef=None, ema=None, ema_decay=None,
                row_len=None, row_active=None):
    """One fused AdamW update of a flat f32 shard: kai0_adamw, or the entry point the optional arguments select.

    ema, ema_decay (together): kai0_adamw_ema / kai0_adamw_rows_ema — master / moments / model copy bit-identical, and in the same
        pass ema += (1 - ema_decay) * (new master - ema) in f32.
    row_len, row_active (together): kai0_adamw_rows / kai0_adamw_rows_ema — the shard is [rows * row_len] with a gradient that is zero
        in most rows (embedding table); bit-identical to the dense form, idle rows cost their gradient read only.  row_active: uint8
        [rows], persistent; with the EMA it must also be set for every row whose ema may differ from its master
        (sharded._sparse_segments builds the flags that way)."""
    WEIGHT_UPDATES[0] += 1
    n = master.numel()
    assert (ema is None) == (ema_decay is None) and (row_len is None) == (row_active is None)
    name, ema_args, ema_tail, size = "kai0_adamw", (), (), (n,)
    if row_len is not None:
        assert n % row_len == 0 and row_active.numel() == n // row_len and row_active.dtype == torch.uint8
        name, size = name + "_rows", (n // row_len, row_len, row_active.data_ptr())
    if ema is not None:
        assert ema.numel() == n and ema.dtype == F32
        name, ema_args, ema_tail = name + "_ema", (ema.data_ptr(),), (float(ema_decay),)
    bc1 = 1.0 - beta1**step
    bc2 = 1.0 - beta2**step
    _lib.call(name, master.data_ptr(), m.data_ptr(), v.data_ptr(), *ema_args, grad.data_ptr(), int(grad.dtype == F32),
              param.data_ptr(), int(param.dtype == F32), *size, lr, beta1, beta2, eps, wd, bc1, bc2, *ema_tail,
              None if clip_coef is None else clip_coef.data_ptr(), _stream())  # fmt: skip


# adamw_step_ under the names, and with the argument order, of the C entry points they select
def adamw_rows_step_(master, m, v, grad, param, row_len: int, row_active, **kw):
    adamw_step_(master, m, v, grad, param, row_len=row_len, row_active=row_active, **kw)


def adamw_ema_step_(master, m, v, ema, grad, param, **kw):
    adamw_step_(master, m, v, grad, param, ema=ema, **kw)


def adamw_rows_ema_step_(master, m, v, ema, grad, param, row_len: int, row_active, **kw):
    adamw_step_(master, m, v, grad, param, ema=ema, row_len=row_len, row_active=row_active, **kw)


def sparse_rows_ok(lr: float, wd: float) -> bool:
    """True if an idle row (zero moments, zero gradient) is a fixed point of the update: 1 - lr*wd rounds to 1 in f32."""
    return bool(np.float32(1.0) - np.float32(lr) * np.float32(wd) == np.float32(1.0))


def check_ema_decay(ema_decay):
    """None (EMA off) or a decay in [0, 1) as a float."""
    if ema_decay is None:
        return None
    d = float(ema_decay)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1) or None, got {ema_decay!r}")
    return d


_SUMSQ_SCRATCH: dict = {}


def sumsq_accumulate_(grad, out):
    """out[0] += sum(grad^2), deterministic (block partials + ordered finish)."""
    key = (grad.device.index, _stream())
    scratch = _SUMSQ_SCRATCH.get(key)
    if scratch is None:
        scratch = _SUMSQ_SCRATCH[key] = torch.empty(4096, dtype=F32, device=grad.device)
    _lib.call("kai0_sumsq", grad.data_ptr(), int(grad.dtype == F32), grad.numel(), out.data_ptr(), scratch.data_ptr(), _stream())


def grad_accum_(acc, grad, *, first: bool, sumsq_out=None):
    """kai0_grad_accum: acc = (0 if first else acc) + grad in f32 (acc f32, grad bf16 or f32, same length; `first` never reads acc);
    with `sumsq_out` also sumsq_out[0] += sum(acc_new^2), deterministic like sumsq_accumulate_, in the same pass."""
    assert acc.dtype == F32 and grad.dtype in (F32, BF16) and acc.numel() == grad.numel()
    scratch = None
    if sumsq_out is not None:
        key = (grad.device.index, _stream())
        scratch = _SUMSQ_SCRATCH.get(key)
        if scratch is None:
            scratch = _SUMSQ_SCRATCH[key] = torch.empty(4096, dtype=F32, device=grad.device)
    _lib.call("kai0_grad_accum", acc.data_ptr(), grad.data_ptr(), int(grad.dtype == F32), acc.numel(), int(bool(first)),
              None if sumsq_out is None else sumsq_out.data_ptr(), None if scratch is None else scratch.data_ptr(), _stream())  # fmt: skip


MAX_MIX_SOURCES = 8  # what one kai0_mix / kai0_multi_dot launch takes


def _src_pointers(srcs, like_numel: int):
    import ctypes as C

    assert 1 <= len(srcs) and all(s.dtype == srcs[0].dtype and s.numel() == like_numel and s.is_contiguous() for s in srcs)
    assert srcs[0].dtype in (F32, BF16)
    return (C.c_void_p * len(srcs))(*(s.data_ptr() for s in srcs))


def mix_(dst, srcs, weights):
    """kai0_mix: dst = w0 * srcs[0] + w1 * srcs[1] + ... in source order, every product and sum rounded to f32 on its own, one rounding
    to dst's dtype.  1..8 sources of one dtype (bf16 or f32) and dst's length; dst (bf16 or f32) may be one of them and is never read."""
    import ctypes as C

    WEIGHT_UPDATES[0] += 1  # dst is usually a model parameter: the write bypasses autograd's version counter
    assert dst.dtype in (F32, BF16) and dst.is_contiguous() and len(weights) == len(srcs)
    ptrs = _src_pointers(srcs, dst.numel())
    w = (C.c_float * len(srcs))(*(float(x) for x in weights))
    _lib.call("kai0_mix", ptrs, int(srcs[0].dtype == F32), w, len(srcs), dst.data_ptr(), int(dst.dtype == F32), dst.numel(), _stream())


_MULTI_DOT_SCRATCH: dict = {}


def multi_dot_(grad, srcs, out):
    """kai0_multi_dot: out[k] += sum(grad * srcs[k]) for the 1..8 sources from one pass over grad; out f64 [len(srcs)] (the caller zeroes
    it), products and block partials f32, partials added in f64 in a fixed order: reproducible bit for bit."""
    assert grad.dtype in (F32, BF16) and grad.is_contiguous() and out.dtype == torch.float64 and out.numel() >= len(srcs) and out.is_contiguous()
    ptrs = _src_pointers(srcs, grad.numel())
    key = (grad.device.index, _stream())
    scratch = _MULTI_DOT_SCRATCH.get(key)
    if scratch is None:
        scratch = _MULTI_DOT_SCRATCH[key] = torch.empty(MAX_MIX_SOURCES * 4096, dtype=F32, device=grad.device)
    _lib.call("kai0_multi_dot", grad.data_ptr(), int(grad.dtype == F32), ptrs, int(srcs[0].dtype == F32), len(srcs), grad.numel(),
              out.data_ptr(), scratch.data_ptr(), _stream())  # fmt: skip


def sum_chunks_(src, chunks: int, out):
    """out[i] = sum_j src[j * out.numel() + i] in f32, one rounding (the local half of the all-pairs reduce-scatter)."""
    n = out.numel()
    assert src.dtype == out.dtype and src.numel() == chunks * n and src.is_contiguous() and out.is_contiguous()
    _lib.call("kai0_sum_chunks", src.data_ptr(), int(src.dtype == F32), int(chunks), n, n, out.data_ptr(), _stream())


def clip_coef_(sumsq, max_norm: float, coef, norm_out):
    _lib.call("kai0_clip_coef", sumsq.data_ptr(), float(max_norm), coef.data_ptr(), norm_out.data_ptr(), _stream())


COEF_SKIP = -1.0  # KAI0_COEF_SKIP (include/kai0hip.h): a negative clip coefficient makes every AdamW form leave everything as it is


def clip_coef_guard_(sumsq, max_norm, coef, norm_out, skipped):
    """kai0_clip_coef_guard: clip_coef_ for a finite norm (max_norm None / <= 0: coef = 1, no clipping); a norm that is inf or NaN writes
    coef = COEF_SKIP — the AdamW launches that follow then change nothing — and adds 1 to `skipped` (int32 [1], on the device)."""
    assert skipped.dtype == torch.int32 and coef.dtype == F32 and norm_out.dtype == F32 and sumsq.dtype == F32
    _lib.call("kai0_clip_coef_guard", sumsq.data_ptr(), float(max_norm or 0.0), coef.data_ptr(), norm_out.data_ptr(), skipped.data_ptr(),
              _stream())  # fmt: skip


class FusedAdamW:
    """torch.optim.AdamW-shaped optimizer (param_groups with "lr", step(), zero_grad(), state_dict()).

    step() = [sum of squared grads over all params -> clip coefficient on device] -> fused AdamW per tensor.
    No host synchronisation: the clip coefficient stays in device memory and is read by the update kernel.
    `ema_decay` (None = off): an f32 EMA of the master copies, state[p]["ema"], updated inside the same kernel (kai0_adamw_ema).
    `skip_nonfinite` (False = off, the launches of before): a step whose global gradient norm is inf or NaN changes nothing — masters,
    moments, EMA and parameters keep their bytes — and is counted in `skipped_steps` (int32 [1], on the device; kai0_clip_coef_guard).
    The norm is then computed even without `max_grad_norm`.  `step_count` advances all the same, so after a skip Adam's bias
    corrections run one step ahead of the number of applied updates (negligible after warm-up; the step stays free of host reads)."""

    def __init__(self, params, lr=2.5e-5, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-10, max_grad_norm=1.0, ema_decay=None,
                 skip_nonfinite=False):
        self.ema_decay = check_ema_decay(ema_decay)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.params = [p for p in params if p.requires_grad]
        # tied parameters appear once
        seen, uniq = set(), []
        for p in self.params:
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        self.params = uniq
        self.param_groups = [{"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay, "params": self.params}]
        self.max_grad_norm = max_grad_norm
        self.step_count = 0
        self.state = {}
        dev = self.params[0].device
        for p in self.params:
            self.state[p] = {
                "master": p.detach().to(F32).clone().contiguous(),
                "exp_avg": torch.zeros(p.shape, dtype=F32, device=p.device),
                "exp_avg_sq": torch.zeros(p.shape, dtype=F32, device=p.device),
            }
            if self.ema_decay is not None:
                self.state[p]["ema"] = self.state[p]["master"].clone()
        self._sumsq = torch.zeros(1, dtype=F32, device=dev)
        self._coef = torch.ones(1, dtype=F32, device=dev)
        self._norm = torch.zeros(1, dtype=F32, device=dev)
        if self.skip_nonfinite:
            self.skipped_steps = torch.zeros(1, dtype=torch.int32, device=dev)

    def master_params(self):
        return [self.state[p]["master"] for p in self.params]

    def ema_params(self):
        """The f32 EMA of every parameter's master copy, in `params` order (needs ema_decay)."""
        if self.ema_decay is None:
            raise RuntimeError("FusedAdamW was built without ema_decay: there is no EMA")
        return [self.state[p]["ema"] for p in self.params]

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self):
        """Returns the (pre-clip) global grad norm as a 1-element device tensor (no sync)."""
        g = self.param_groups[0]
        lr, (b1, b2), eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        self.step_count += 1
        live = [p for p in self.params if p.grad is not None]
        coef = None
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self._sumsq.zero_()
            for p in live:
                sumsq_accumulate_(p.grad.contiguous(), self._sumsq)
            if self.skip_nonfinite:
                clip_coef_guard_(self._sumsq, self.max_grad_norm, self._coef, self._norm, self.skipped_steps)
            else:
                clip_coef_(self._sumsq, self.max_grad_norm, self._coef, self._norm)
            coef = self._coef
        for p in live:
            st = self.state[p]
            adamw_step_(st["master"], st["exp_avg"], st["exp_avg_sq"], p.grad.contiguous(), p.data, lr=lr, beta1=b1, beta2=b2, eps=eps,
                        wd=wd, step=self.step_count, clip_coef=coef, ema=st.get("ema"), ema_decay=self.ema_decay)  # fmt: skip
        return self._norm

    def state_dict(self):
        return {
            "step": self.step_count,
            "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}],
            "state": [{k: v for k, v in self.state[p].items()} for p in self.params],
            **({"skipped_steps": int(self.skipped_steps)} if self.skip_nonfinite else {}),
        }

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        if self.skip_nonfinite:  # absent in a state written without the guard: 0
            self.skipped_steps.fill_(int(sd.get("skipped_steps", 0)))
        for k, v in sd["param_groups"][0].items():
            self.param_groups[0][k] = v
        for p, st in zip(self.params, sd["state"], strict=True):
            for k in ("master", "exp_avg", "exp_avg_sq"):
                self.state[p][k].copy_(st[k])
            if self.ema_decay is not None:  # a state written without EMA: the average starts from the master
                self.state[p]["ema"].copy_(st["ema"] if "ema" in st else st["master"])
