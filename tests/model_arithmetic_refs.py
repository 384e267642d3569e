"""Restatements shared by tests/test_model_arithmetic_cpu.py and tests/test_model_arithmetic_gpu.py: the arithmetic contract of
`kai0_mix` in torch ops, torch stand-ins for the two hooks of `kai0_amd.model_arithmetic.CheckpointSet`, and the launch arithmetic
of `kai0_multi_dot` (csrc/optim.hip) from which the tests derive their bound."""

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def mix_restated(srcs, weights, out_dtype):
    """acc = w0 * x0; acc = acc + w1 * x1; ... in source order — torch's eager mul and add round every product and every sum on
    their own (nothing is fused) — then ONE rounding to out_dtype.  f32 arithmetic with f32 weights; for a float64 destination
    (the CPU tests' float64 models) the same chain in float64."""
    ct = F64 if out_dtype == F64 else F32
    w = torch.tensor([float(x) for x in weights], dtype=F64).to(ct).to(srcs[0].device)
    acc = srcs[0].to(ct) * w[0]
    for k in range(1, len(srcs)):
        acc = acc + srcs[k].to(ct) * w[k]
    return acc.to(out_dtype)


class TorchArithmeticOps:
    """Stand-ins for HipArithmeticOps: `mix` is the restatement above, `multi_dot` the float64 inner products.  Counts its calls."""

    def __init__(self):
        self.mixes, self.dots, self.max_sources = [], [], 0

    def mix(self, dst, srcs, weights):
        assert 1 <= len(srcs) <= 8 and len(weights) == len(srcs)
        self.mixes.append(dst.data_ptr())
        dst.copy_(mix_restated(srcs, weights, dst.dtype).view_as(dst))

    def multi_dot(self, grad, srcs, out):
        assert 1 <= len(srcs) <= 8 and out.dtype == F64 and out.numel() == len(srcs)
        self.dots.append(grad.data_ptr())
        self.max_sources = max(self.max_sources, len(srcs))
        for k, s in enumerate(srcs):
            out[k] += (grad.to(F64) * s.to(F64)).sum()


def multi_dot_launch(n: int, g_ptr: int, gsz: int, src_ptrs, ssz: int):
    """(head, blocks, T) of kai0_multi_dot, from n and the pointers alone (include/kai0hip.h, csrc/optim.hip):
      head   = elements up to g's first 4-element boundary (16 B f32, 8 B bf16) if every source reaches ITS boundary at the same
               element, else n (everything scalar);  n4 = (n - head) // 4 vectors, rest = n - 4 n4 scalar elements
      blocks = min(ceil(n4 / 256), 4096), at least min(max(ceil(rest / 256), 1), 4096)
      every block takes ceil(n4 / blocks) consecutive vectors, a lane every 256th of them; the scalar elements are grid-strided.
    T = the most products one lane adds: 4 per vector it takes plus its scalar elements."""
    head = min(((4 * gsz - g_ptr % (4 * gsz)) % (4 * gsz)) // gsz, n)
    if any((p + head * ssz) % (4 * ssz) for p in src_ptrs):
        head = n
    n4 = (n - head) // 4
    rest = n - 4 * n4
    blocks = max(min(-(-n4 // 256), 4096), min(max(-(-rest // 256), 1), 4096))
    per = -(-n4 // blocks)
    return head, blocks, 4 * -(-per // 256) + -(-rest // (blocks * 256))


def multi_dot_bound(T: int, abs_sum: float) -> float:
    """(T + 12) 2^-24 sum|g x|: a lane's chain is T products (one rounding each; exact for bf16 x bf16) and T additions, the wave's
    shuffle tree adds 6 levels, the four wave partials 4 more — T + 11 roundings of at most 2^-24 relative to the sum of magnitudes to
    first order, one kept for the second-order terms; the float64 finish adds nothing at this scale."""
    return (T + 12) * 2.0**-24 * abs_sum
