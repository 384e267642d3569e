"""Model arithmetic on the MI355X: `kai0_mix` bit for bit against its f32 restatement computed on the CPU, `kai0_multi_dot` against
float64 within a bound derived from its launch arithmetic (tests/model_arithmetic_refs.py), and `kai0_amd.model_arithmetic` on the
tiny model of tests/tiny.py: mixing, projection, teacher-forced optimiser iterations, the inference engine after a merge."""

import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from model_arithmetic_refs import BF16, F32, F64, TorchArithmeticOps, mix_restated, multi_dot_bound, multi_dot_launch  # noqa: E402
from streaming_refs import GUARD, SENTINEL  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def P(t):
    return t.data_ptr()


def ptr_array(tensors):
    import ctypes as C

    return (C.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


def f32_array(values):
    import ctypes as C

    return (C.c_float * len(values))(*values)


def call(name, *args):
    from kai0_amd import _lib

    _lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


class Band:
    """A length-n view starting GUARD + off elements into a fresh (16-byte aligned) buffer of sentinels."""

    def __init__(self, n, dtype, off=0, init=None, fill=NAN):
        self.buf = torch.full((n + off + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD + off : GUARD + off + n]
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        self.lo, self.hi = GUARD + off, GUARD + off + n
        if init is not None:
            self.t.copy_(init)
        else:
            self.t.fill_(fill)

    def check(self, what):
        assert bool((self.buf[: self.lo] == SENTINEL).all()) and bool((self.buf[self.hi :] == SENTINEL).all()), f"{what}: wrote outside its view"


# ================================================================================================ 1. kai0_mix, bit-exact
MIX_SIZES = [1, 7, 8, 1027, 256 * 1024 * 4 + 5]
MIX_WEIGHTS = [0.75, -0.5, 0.0, 1.25, 0.3, -0.1, 0.6, 0.2]  # a zero, negative values, sum 2.5
# (source, destination) element offsets from a 16-byte boundary: aligned; both one in (same dtype: a common scalar head of 3 / 7
# elements, then 16-byte accesses; f32 sources into bf16: a common head of 7; bf16 sources into f32: none, scalar throughout); only the
# sources; only the destination (both scalar throughout)
MIX_LAYOUTS = {"aligned": (0, 0), "together": (1, 1), "sources": (1, 0), "destination": (0, 1)}
_SRC_CACHE = {}


def mix_sources(dtype):
    """Eight CPU tensors of the largest size, made once per dtype; every case takes a prefix."""
    if dtype not in _SRC_CACHE:
        g = torch.Generator().manual_seed(11)
        _SRC_CACHE[dtype] = [(torch.randn(MIX_SIZES[-1], generator=g) * (0.5 + k)).to(dtype) for k in range(8)]
    return _SRC_CACHE[dtype]


@pytest.mark.parametrize("dst_dtype", [BF16, F32])
@pytest.mark.parametrize("src_dtype", [BF16, F32])
@pytest.mark.parametrize("n_src", [1, 2, 3, 8])
def test_mix_is_the_f32_chain_bit_for_bit(n_src, src_dtype, dst_dtype):
    """acc = w0 x0; acc = acc + w1 x1; ... with every product and sum rounded to f32, one rounding to the destination: torch.equal
    to the CPU restatement for every size and layout, from a destination full of NaN between intact sentinels; sources only read."""
    w = MIX_WEIGHTS[:n_src]
    for n in MIX_SIZES:
        cpu = [s[:n] for s in mix_sources(src_dtype)[:n_src]]
        want = mix_restated(cpu, w, dst_dtype)
        assert not bool(torch.isnan(want).any())
        on_dev = [c.to(DEV) for c in cpu]
        for layout, (so, do) in MIX_LAYOUTS.items():
            srcs = [Band(n, src_dtype, so, init=c) for c in on_dev]
            dst = Band(n, dst_dtype, do)
            call("kai0_mix", ptr_array([s.t for s in srcs]), int(src_dtype == F32), f32_array(w), n_src, P(dst.t), int(dst_dtype == F32), n)
            torch.cuda.synchronize()
            got = dst.t.cpu()
            what = f"N={n_src} {src_dtype}->{dst_dtype} n={n} {layout}"
            assert int(torch.isnan(got).sum()) == 0, f"{what}: NaN left in the destination"
            assert torch.equal(got, want), f"{what}: {int((got != want).sum())} elements differ"
            dst.check(what)
            for s, c in zip(srcs, on_dev):
                s.check(what)
                assert torch.equal(s.t, c), f"{what}: a source changed"


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n_src", [1, 3, 8])
def test_mix_into_its_first_source(n_src, dtype):
    """dst aliasing source 0 (what a merge into a resident checkpoint does): the same result as into a fresh buffer."""
    w = MIX_WEIGHTS[:n_src]
    for n in MIX_SIZES:
        cpu = [s[:n] for s in mix_sources(dtype)[:n_src]]
        want = mix_restated(cpu, w, dtype)
        for off in (0, 1):
            srcs = [Band(n, dtype, off, init=c) for c in cpu]
            call("kai0_mix", ptr_array([s.t for s in srcs]), int(dtype == F32), f32_array(w), n_src, P(srcs[0].t), int(dtype == F32), n)
            torch.cuda.synchronize()
            assert torch.equal(srcs[0].t.cpu(), want), f"N={n_src} {dtype} n={n} off={off}"
            for s, c in zip(srcs[1:], cpu[1:]):
                assert torch.equal(s.t.cpu(), c)
            for s in srcs:
                s.check("alias")


def test_mix_argument_checks():
    """n_src outside 1..8, a non-finite weight, a null or misaligned pointer: an error with a message and nothing launched (the
    destination keeps its NaN); n = 0 is a no-op; the hook in kai0_amd.optim reaches the same kernel."""
    from kai0_amd import _lib, optim

    n = 64
    srcs = [torch.ones(n, device=DEV) for _ in range(9)]
    dst = torch.full((n,), NAN, device=DEV)
    ok = ptr_array(srcs)
    odd = ptr_array(srcs[:2])
    odd[1] = srcs[1].data_ptr() + 2
    null = ptr_array(srcs[:2])
    null[1] = None
    for args, msg in (((ok, 1, f32_array([1.0] * 9), 0, P(dst), 1, n), "n_src = 0 outside 1..8"),
                      ((ok, 1, f32_array([1.0] * 9), 9, P(dst), 1, n), "n_src = 9 outside 1..8"),
                      ((ok, 1, f32_array([1.0, NAN]), 2, P(dst), 1, n), "weight 1 is not finite"),
                      ((ok, 1, f32_array([float("inf"), 1.0]), 2, P(dst), 1, n), "weight 0 is not finite"),
                      ((odd, 1, f32_array([1.0, 1.0]), 2, P(dst), 1, n), "not aligned to its element size"),
                      ((ok, 1, f32_array([1.0, 1.0]), 2, P(dst) + 2, 1, n - 1), "not aligned to its element size"),
                      ((ok, 0, f32_array([1.0, 1.0]), 2, P(dst) + 1, 0, n), "not aligned to its element size"),
                      ((null, 1, f32_array([1.0, 1.0]), 2, P(dst), 1, n), "null buffer"),
                      ((ok, 1, f32_array([1.0, 1.0]), 2, None, 1, n), "null buffer"),
                      ((ok, 1, None, 2, P(dst), 1, n), "null buffer")):  # fmt: skip
        with pytest.raises(_lib.Kai0HipError, match=msg):
            call("kai0_mix", *args)
    call("kai0_mix", None, 1, None, 0, None, 1, 0)  # n <= 0: nothing to do, nothing checked
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())
    before = optim.WEIGHT_UPDATES[0]
    optim.mix_(dst, srcs[:3], [0.5, 0.25, 2.0])
    torch.cuda.synchronize()
    assert torch.equal(dst, torch.full((n,), 2.75, device=DEV)) and optim.WEIGHT_UPDATES[0] == before + 1


# ================================================================================================ 2. kai0_multi_dot
DOT_SIZES = [1, 1027, 4096 * 1024 + 1029]  # the last: 1048833 vectors for 4096 x 256 lanes — lane 0 of every block takes a second one
DOT_LAYOUTS = {"aligned": (0, 0), "together": (1, 1), "separately": (1, 0)}  # (g, sources) element offsets


def dot_inputs(n, n_src, g_dtype, s_dtype):
    """g random; x_k = +-g in alternating runs of 64 (k + 1) elements (4 (k + 1) at the small sizes, so that the unpaired last runs
    stay a small share of n) plus a small independent part: sum g x_k cancels to a small fraction of sum |g x_k|, so an error of the
    size the bound allows would show."""
    g = torch.Generator(device=DEV).manual_seed(5)
    gv = (torch.randn(n, generator=g, device=DEV) * 2).to(g_dtype)
    j = torch.arange(n, device=DEV)
    xs = []
    for k in range(n_src):
        sign = 1.0 - 2.0 * ((j // ((64 if n > 2**16 else 4) * (k + 1))) % 2).to(F32)
        xs.append((gv.to(F32) * sign + 0.01 * torch.randn(n, generator=g, device=DEV)).to(s_dtype))
    return gv, xs


@pytest.mark.parametrize("s_dtype", [BF16, F32])
@pytest.mark.parametrize("g_dtype", [BF16, F32])
@pytest.mark.parametrize("n_src", [1, 3, 8])
def test_multi_dot_within_its_derived_bound(n_src, g_dtype, s_dtype):
    """out[k] += sum_j g_j x_kj against float64 within (T + 12) 2^-24 sum_j |g_j x_kj| (T from the launch arithmetic, not from the
    result), on cancelling inputs; two calls agree bit for bit; a second call without zeroing doubles `out` exactly; partials land in
    scratch[k * 4096 + block] only — nothing beyond n_src * 4096 floats, nothing outside `out`."""
    for n in DOT_SIZES:
        gv, xs = dot_inputs(n, n_src, g_dtype, s_dtype)
        ref = [float((gv.to(F64) * x.to(F64)).sum()) for x in xs]
        mag = [float((gv.to(F64) * x.to(F64)).abs().sum()) for x in xs]
        for layout, (go, so) in DOT_LAYOUTS.items():
            g = Band(n, g_dtype, go, init=gv)
            srcs = [Band(n, s_dtype, so, init=x) for x in xs]
            head, blocks, T = multi_dot_launch(n, P(g.t), g.t.element_size(), [P(s.t) for s in srcs], srcs[0].t.element_size())
            if n >= 4:
                assert head == {"aligned": 0, "together": 3, "separately": n}[layout]  # (4-element vectors whatever the dtypes)
            if n > 2**22 and head < n:
                assert blocks == 4096 and T == 8 + 1
            res = []
            for _ in range(2):
                out, scratch = Band(n_src, F64, fill=0.0), Band(n_src * 4096, F32)
                args = (P(g.t), int(g_dtype == F32), ptr_array([s.t for s in srcs]), int(s_dtype == F32), n_src, n, P(out.t), P(scratch.t))
                call("kai0_multi_dot", *args)
                torch.cuda.synchronize()
                res.append(out.t.clone())
            assert torch.equal(res[0], res[1]), "two calls differ"
            call("kai0_multi_dot", *args)  # out +=
            torch.cuda.synchronize()
            assert torch.equal(out.t, res[0] + res[0])
            out.check("out"), scratch.check("scratch"), g.check("g")
            part = scratch.t.view(n_src, 4096)
            assert int(torch.isnan(part[:, :blocks]).sum()) == 0 and bool(torch.isnan(part[:, blocks:]).all())
            worst = 0.0
            for k in range(n_src):
                bnd = multi_dot_bound(T, mag[k])
                worst = max(worst, abs(float(res[0][k]) - ref[k]) / bnd)
                assert abs(ref[k]) < 0.2 * mag[k] or n < 128  # it cancels
            print(f"multi_dot N={n_src} g {g_dtype} x {s_dtype} n={n} {layout}: T={T} blocks={blocks} worst error/bound {worst:.3f}")
            assert worst <= 1.0
            for s, x in zip(srcs, xs):
                s.check("source")
                assert torch.equal(s.t, x)


def test_multi_dot_argument_checks():
    from kai0_amd import _lib, optim

    n = 64
    g = torch.ones(n, device=DEV)
    srcs = [torch.full((n,), float(k + 1), device=DEV) for k in range(9)]
    out = torch.zeros(9, dtype=F64, device=DEV)
    scratch = torch.full((8 * 4096,), NAN, device=DEV)
    ok = ptr_array(srcs)
    odd = ptr_array(srcs[:2])
    odd[0] = srcs[0].data_ptr() + 1
    for args, msg in (((P(g), 1, ok, 1, 0, n, P(out), P(scratch)), "n_src = 0 outside 1..8"),
                      ((P(g), 1, ok, 1, 9, n, P(out), P(scratch)), "n_src = 9 outside 1..8"),
                      ((None, 1, ok, 1, 2, n, P(out), P(scratch)), "null buffer"),
                      ((P(g), 1, ok, 1, 2, n, None, P(scratch)), "null buffer"),
                      ((P(g), 1, ok, 1, 2, n, P(out), None), "scratch"),
                      ((P(g) + 2, 1, ok, 1, 2, n - 1, P(out), P(scratch)), "not aligned to its element size"),
                      ((P(g), 1, ok, 1, 2, n, P(out) + 4, P(scratch)), "not aligned to its element size"),
                      ((P(g), 1, odd, 0, 2, n, P(out), P(scratch)), "not aligned to its element size")):  # fmt: skip
        with pytest.raises(_lib.Kai0HipError, match=msg):
            call("kai0_multi_dot", *args)
    call("kai0_multi_dot", None, 1, None, 1, 0, 0, None, None)  # n <= 0: nothing to do, nothing checked
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and bool(torch.isnan(scratch).all())
    optim.multi_dot_(g, srcs[:3], out[:3])
    optim.multi_dot_(g.to(BF16), [s.to(BF16) for s in srcs[3:5]], out[3:5])
    torch.cuda.synchronize()
    assert out.tolist() == [64.0, 128.0, 192.0, 256.0, 320.0, 0.0, 0.0, 0.0, 0.0]


# ================================================================================================ 3. the tiny model
@pytest.fixture(scope="module")
def tiny():
    """The tiny model, three perturbed copies of its state dict (CPU, parameter dtypes), one batch with fixed noise and time."""
    from tiny import build_pair, obs_to

    from oracle.pi0_oracle import synthetic_batch

    dev = torch.device(DEV)
    model, _, _, ocfg = build_pair(dev, seed=0, std=0.08)
    base = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(21)
    sds = []
    for k in range(3):
        sds.append({n: (t.float() * (1.0 + 0.05 * torch.randn(t.shape, generator=g)) + 0.002 * torch.randn(t.shape, generator=g)).to(t.dtype)
                    if t.is_floating_point() else t.clone() for n, t in base.items()})  # fmt: skip
    obs, actions, noise, time = synthetic_batch(ocfg, 2, seed=0)
    batch = (obs_to(obs, dev), actions.to(dev))
    return dict(model=model, base=base, sds=sds, batch=batch, noise=noise.to(dev), time=time.to(dev), dev=dev)


def _source(cs, sds, name, k):
    """Source k of parameter `name` as the CheckpointSet keeps it: on the CPU, in the parameter's dtype."""
    i = cs.names.index(name)
    return cs.sources[i][k].cpu()


def _dot_bound_for(cs):
    """Per source: sum over the parameters with a gradient of the kernel's bound for that call, and the float64 reference."""
    ref = [0.0] * cs.n
    bnd = [0.0] * cs.n
    for p, srcs in zip(cs.params, cs.sources):
        if p.grad is None:
            continue
        g = p.grad.detach().contiguous()
        _, _, T = multi_dot_launch(g.numel(), g.data_ptr(), g.element_size(), [s.data_ptr() for s in srcs], srcs[0].element_size())
        for k, s in enumerate(srcs):
            prod = g.to(F64) * s.to(F64)
            ref[k] += float(prod.sum())
            bnd[k] += multi_dot_bound(T, float(prod.abs().sum()))
    return ref, bnd


def test_model_mix_into_equals_the_per_tensor_restatement(tiny):
    from kai0_amd import model_arithmetic as ma

    model = tiny["model"]
    cs = ma.CheckpointSet(model, tiny["sds"])
    assert len(cs.params) == len(list(model.parameters())) and not cs.skipped
    w32 = cs.mix_into([0.5, 0.2, 0.3])
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        want = mix_restated([_source(cs, tiny["sds"], name, k) for k in range(3)], w32, p.dtype)
        assert torch.equal(p.detach().cpu(), want.view_as(p)), name
    dtypes = {p.dtype for p in model.parameters()}
    assert BF16 in dtypes and F32 in dtypes  # both destination forms ran


def test_model_projection_and_teacher_forced_iterations(tiny):
    """Five iterations of the gradient-descent loop, teacher-forced: every iteration starts from the log-weights of a restatement whose
    mixing and projection are torch ops on the same model (TorchArithmeticOps), so no trajectory tolerance is needed — the mixed
    parameters are bit-identical, hence the losses are; g_k is compared within the kernel's bound summed over the parameters, against
    float64 inner products of the SAME gradients."""
    from kai0_amd import model_arithmetic as ma

    model, batch, noise, time = tiny["model"], tiny["batch"], tiny["noise"], tiny["time"]
    model.train()
    hip = ma.CheckpointSet(model, tiny["sds"])
    ref = ma.CheckpointSet(model, tiny["sds"], ops=TorchArithmeticOps())
    log_w = torch.zeros(3, dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([log_w], lr=0.1)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5, eta_min=0.001)
    for it in range(5):
        w = torch.softmax(log_w.detach(), 0)
        loss_h, g_h, _ = ma.projected_gradient(hip, w, batch, noise=noise, time=time)
        mixed_h = [p.detach().clone() for p in model.parameters()]
        g_ref, bnd = _dot_bound_for(hip)  # from the gradients the HIP iteration left in place
        ratios = [abs(float(g_h[k]) - g_ref[k]) / bnd[k] for k in range(3)]
        print(f"iteration {it}: loss {loss_h!r}, g {[float(x) for x in g_h]}, worst error/bound {max(ratios):.3f}")
        assert max(ratios) <= 1.0 and all(abs(x) > 0 for x in g_ref)
        assert ref.project() == pytest.approx(g_ref, rel=1e-12)  # the stand-in states the same inner products
        loss_r, g_r, grad_r = ma.projected_gradient(ref, w, batch, noise=noise, time=time)
        assert all(torch.equal(a, b) for a, b in zip(mixed_h, model.parameters())), "the mixed parameters differ"
        assert loss_r == loss_h, (it, loss_r, loss_h)
        log_w.grad = grad_r
        opt.step()
        opt.zero_grad(set_to_none=True)
        sched.step()
    assert float((torch.softmax(log_w.detach(), 0) - 1 / 3).abs().max()) > 1e-3  # the restatement's weights moved
    model.zero_grad(set_to_none=True)
    model.eval()


def test_model_engine_is_dropped_by_mix_into(tiny):
    """An engine captured on the unmixed weights, then mix_into: sample_actions must equal, bit for bit, that of a fresh model
    that received the same mixed tensors through load_state_dict."""
    from tiny import tiny_cfgs

    from kai0_amd import model_arithmetic as ma
    from kai0_amd.model import PI0Pytorch

    model, dev, (gobs, _), noise = tiny["model"], tiny["dev"], tiny["batch"], tiny["noise"]
    model.load_state_dict(tiny["base"])
    model.eval()
    before = model.sample_actions(dev, gobs, noise=noise, num_steps=10)
    assert model._engine is not None
    cs = ma.CheckpointSet(model, tiny["sds"])
    cs.mix_into([0.1, 0.6, 0.3])
    assert model._engine is None
    after = model.sample_actions(dev, gobs, noise=noise, num_steps=10)
    fresh = PI0Pytorch(tiny_cfgs()[0])
    fresh.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    want = fresh.sample_actions(dev, gobs, noise=noise, num_steps=10)
    torch.cuda.synchronize()
    assert torch.equal(after, want)
    assert not torch.equal(after, before)
