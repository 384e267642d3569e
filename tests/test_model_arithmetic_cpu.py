"""kai0_amd.model_arithmetic on the CPU: the whole host module over torch stand-ins for its two kernels (tests/model_arithmetic_refs.py),
the same idea as the sharded engine over `TorchShardOps`.  The kernels themselves: tests/test_model_arithmetic_gpu.py."""

import json
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch.func import functional_call

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from model_arithmetic_refs import BF16, F32, F64, TorchArithmeticOps, mix_restated  # noqa: E402

from kai0_amd import model_arithmetic as ma  # noqa: E402


# ================================================================================================ the stand-in mix
@pytest.mark.parametrize("out_dtype", [F32, BF16])
@pytest.mark.parametrize("src_dtype", [F32, BF16])
@pytest.mark.parametrize("n_src", [1, 2, 3, 8])
def test_restated_mix_against_float64_average(n_src, src_dtype, out_dtype):
    """The f32 restatement (the contract kai0_mix is held to bit for bit) against the reference's float64 np.average
    (common.py:17-18): N roundings of products and sums of at most 2^-24 each relative to sum|w_k x_k| to first order — N 2^-23 allows
    twice that — plus half an ulp of the output dtype (2^-24 / 2^-8 relative) for the one rounding of the accumulated value.
    np.average divides by sum(w); the weights here are normalised before their f32 rounding, and the average is multiplied back by
    that sum so that both sides state sum_k w_k x_k for the SAME f32 weights."""
    g = torch.Generator().manual_seed(n_src)
    srcs = [(torch.randn(4099, generator=g) * 3).to(src_dtype) for _ in range(n_src)]
    w = torch.rand(n_src, generator=g, dtype=F64) + 0.05
    w32 = (w / w.sum()).to(F32)
    got = mix_restated(srcs, w32.tolist(), out_dtype).to(F64).numpy()
    w64 = w32.to(F64).numpy()
    stacked = np.stack([s.to(F64).numpy() for s in srcs], axis=0)
    ref = np.average(stacked, axis=0, weights=w64) * w64.sum()
    mag = np.abs(stacked * w64[:, None]).sum(axis=0)
    acc_err = n_src * 2.0**-23 * mag
    bound = acc_err + (2.0**-24 if out_dtype == F32 else 2.0**-8) * (np.abs(ref) + acc_err)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"restated mix vs float64 average, N={n_src} {src_dtype}->{out_dtype}: worst error/bound {ratio:.3f}")
    assert ratio <= 1.0


# ================================================================================================ a small smooth model
class Net(torch.nn.Module):
    """float64; `head.weight` is tied to `embed` (one parameter under two names, like embed_tokens / lm_head)."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.embed = torch.nn.Parameter(torch.randn(6, 5, generator=g, dtype=F64) * 0.5)
        self.l1 = torch.nn.Linear(5, 7, dtype=F64)
        self.head = torch.nn.Linear(5, 6, bias=False, dtype=F64)
        self.head.weight = self.embed
        self.scale = torch.nn.Parameter(torch.ones(7, dtype=F64))
        with torch.no_grad():
            self.l1.weight.copy_(torch.randn(7, 5, generator=g, dtype=F64) * 0.4)
            self.l1.bias.copy_(torch.randn(7, generator=g, dtype=F64) * 0.1)

    def forward(self, x):
        h = torch.tanh(self.l1(x @ self.embed)) * self.scale
        return h.sum(-1, keepdim=True) * self.head(x @ self.embed)


def net_loss(model, batch, noise=None, time=None):
    x, y = batch
    return ((model(x) - y) ** 2).mean()


def perturbed(model, k, scale=0.3):
    g = torch.Generator().manual_seed(100 + k)
    sd = {n: t.detach().clone() + scale * torch.randn(t.shape, generator=g, dtype=t.dtype) for n, t in model.state_dict().items()}
    if "head.weight" in sd:
        sd["head.weight"] = sd["embed"]  # one tensor under two names
    return sd


def batches(n=2, big_second=False):
    g = torch.Generator().manual_seed(7)
    out = []
    for i in range(n):
        x = torch.randn(9, 6, generator=g, dtype=F64)
        y = torch.randn(9, 6, generator=g, dtype=F64) * (10.0 if big_second and i % 2 else 1.0)
        out.append((x, y))
    return out


def autograd_loss(model, sds, log_w, batch):
    """loss(softmax(log_w)-mixed parameters), differentiable in log_w."""
    w = torch.softmax(log_w, dim=0)
    mixed = {n: sum(w[k] * sds[k][n] for k in range(len(sds))) for n in sds[0] if n != "head.weight"}  # (tied to "embed")
    return net_loss(lambda x: functional_call(model, mixed, (x,)), batch)


def test_projected_gradient_is_the_gradient_with_respect_to_the_log_weights():
    """w (g_k - sum_j w_j g_j) from project() against autograd's d loss / d log_w through softmax and the mix, float64, 1e-9 relative.
    mix_into rounds its weights to f32 on the host (2^-24 relative, far above 1e-9), so the point is chosen with dyadic weights
    (1/2, 1/8, 3/8): the f32 rounding returns them exactly and both sides evaluate the same function at the same point."""
    model, bs = Net(), batches()
    sds = [perturbed(model, k) for k in range(3)]
    cs = ma.CheckpointSet(model, sds, ops=TorchArithmeticOps())
    log_w = (torch.log(torch.tensor([0.5, 0.125, 0.375], dtype=F64)) + 0.7).requires_grad_(True)
    ref_loss = autograd_loss(model, sds, log_w, bs[0])
    (ref_grad,) = torch.autograd.grad(ref_loss, log_w)
    loss, g, grad = ma.projected_gradient(cs, torch.softmax(log_w.detach(), 0), bs[0], loss_fn=net_loss)
    assert abs(loss - float(ref_loss.detach())) <= 1e-12 * abs(float(ref_loss.detach()))
    assert float(ref_grad.abs().max()) > 1e-3 and len(g) == 3
    assert torch.allclose(grad, ref_grad, rtol=1e-9, atol=1e-9 * float(ref_grad.abs().max())), (grad, ref_grad)
    _, _, grad_a = ma.projected_gradient(cs, torch.softmax(log_w.detach(), 0), bs[0], loss_fn=net_loss, adaptive=True)
    assert torch.allclose(grad_a, ref_grad * (float(ref_loss.detach()) / 0.05) ** 2, rtol=1e-9, atol=0)


@pytest.mark.parametrize("adaptive", [False, True])
def test_gradient_descent_trajectory_equals_adam_on_the_autograd_gradient(adaptive):
    """10 iterations against a straight restatement: torch.optim.Adam + CosineAnnealingLR (eta_min = 1 % of the rate) on log-weights
    whose gradient autograd takes through softmax and the mix (times (loss / 0.05)^2 if adaptive), batch `it % len(batches)`.  The
    second batch's targets are 10 x larger, so the odd iterations — the last one too — have the larger losses: the returned weights
    must be those of the best iteration, not of the last."""
    model, bs = Net(), batches(2, big_second=True)
    sds = [perturbed(model, k) for k in range(3)]
    lr, iters = (0.05, 10) if adaptive else (0.5, 10)
    history = []
    got = ma.optimize_gradient_descent(ma.CheckpointSet(model, sds, ops=TorchArithmeticOps()), bs, num_iterations=iters, learning_rate=lr,
                                       adaptive=adaptive, loss_fn=net_loss, history=history)  # fmt: skip
    log_w = torch.zeros(3, dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([log_w], lr=lr)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=iters, eta_min=lr * 0.01)
    ref = []
    for it in range(iters):
        loss = autograd_loss(model, sds, log_w, bs[it % 2])
        ref.append((float(loss.detach()), torch.softmax(log_w.detach(), 0).tolist()))
        opt.zero_grad()
        loss.backward()
        if adaptive:
            log_w.grad.mul_((float(loss.detach()) / 0.05) ** 2)
        opt.step()
        sched.step()
    assert len(history) == iters
    assert np.allclose([h[1] for h in history], [r[1] for r in ref], rtol=1e-6, atol=1e-6)
    assert np.allclose([h[0] for h in history], [r[0] for r in ref], rtol=1e-6, atol=0)
    assert max(abs(a - b) for a, b in zip(ref[0][1], ref[-1][1])) > 1e-2  # the weights moved
    best = min(range(iters), key=lambda i: history[i][0])
    assert best % 2 == 0 and best != iters - 1
    assert got == history[best][1] and got != history[-1][1]


# ================================================================================================ greedy
class Point(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.theta = torch.nn.Parameter(torch.zeros(2, dtype=F64))


def test_greedy_picks_the_best_addition_and_stops_when_none_improves():
    """loss = |theta|^2 with checkpoints c0 = (1, 0), c1 = (1.1, 0.1), c2 = (-1.2, 0), c3 = (5, 5): the two best singles are c0 and c1,
    but c1 only makes c0 worse while c2 nearly cancels it — greedy must take {c0, c2}; no third checkpoint improves 0.01, so it stops
    there, after 4 + 3 + 2 evaluations, with weights 1/2 on the selected."""
    calls = []

    def loss_fn(model, batch, noise=None, time=None):
        calls.append(model.theta.detach().clone())
        return (model.theta**2).sum()

    pts = [(1.0, 0.0), (1.1, 0.1), (-1.2, 0.0), (5.0, 5.0)]
    cs = ma.CheckpointSet(Point(), [{"theta": torch.tensor(p, dtype=F64)} for p in pts], ops=TorchArithmeticOps())
    assert ma.checkpoint_losses(cs, [None], loss_fn=loss_fn) == pytest.approx([1.0, 1.22, 1.44, 50.0], rel=1e-12)
    calls.clear()
    w = ma.optimize_greedy(cs, [None, None], loss_fn=loss_fn)
    assert w == [0.5, 0.0, 0.5, 0.0]
    assert len(calls) == 2 * (4 + 3 + 2)  # two batches per evaluation
    assert torch.allclose(calls[-1], torch.tensor([(1.0 - 1.2 + 5.0) / 3, 5.0 / 3], dtype=F64), rtol=1e-6)  # the last try: {c0, c2, c3}


# ================================================================================================ weights, norm stats, files
def test_inverse_loss_weights_and_norm_stats():
    losses = [0.02, 0.05, 0.01]
    inv = [(1.0 / (l + 1e-8)) ** 2 for l in losses]
    assert ma.inverse_loss_weights(losses) == pytest.approx([v / sum(inv) for v in inv], rel=1e-12)
    a = {"state": {"mean": [1.0, 2.0], "std": [1.0, 1.0]}, "tag": "first"}
    b = {"state": {"mean": [3.0, 6.0], "std": [3.0, 1.0]}, "tag": "second"}
    mixed = ma.mix_norm_stats([a, b], weights=[3.0, 1.0])  # renormalised to 0.75 / 0.25
    assert mixed == {"state": {"mean": [1.5, 3.0], "std": [1.5, 1.0]}, "tag": "first"}
    assert ma.mix_norm_stats([a, b])["state"]["mean"] == [2.0, 4.0]
    assert ma.mix_norm_stats([b], weights=[2.0]) is b


class Mixed(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(3, 4, dtype=BF16))
        self.b = torch.nn.Parameter(torch.zeros(5, dtype=F32))
        self.register_buffer("steps", torch.tensor(3))


@pytest.mark.parametrize("as_float32", [False, True])
def test_save_mixed_round_trip(tmp_path, as_float32):
    """Checkpoint directories in, a directory out: model.safetensors holds the mixed tensors in the parameters' dtypes (or float32),
    norm_stats.json sits beside it in the reference's {"norm_stats": ...} envelope; `params` child directories resolve."""
    from safetensors.torch import load_file, save_file

    g = torch.Generator().manual_seed(0)
    sds = []
    for k in range(2):
        sd = {"a": torch.randn(3, 4, generator=g).to(BF16), "b": torch.randn(5, generator=g)}
        d = tmp_path / f"ckpt{k}"
        (d / "params").mkdir(parents=True)
        save_file(sd, str(d / "model.safetensors"))
        sds.append(sd)
    assert ma.resolve_torch_ckpt_path(tmp_path / "ckpt0" / "params") == str((tmp_path / "ckpt0").resolve())
    with pytest.raises(FileNotFoundError):
        ma.resolve_torch_ckpt_path(tmp_path)
    model = Mixed()
    cs = ma.CheckpointSet(model, [str(tmp_path / "ckpt0"), str(tmp_path / "ckpt1" / "params")], ops=TorchArithmeticOps())
    w32 = cs.mix_into([3.0, 1.0], normalize=True)
    assert w32 == [0.75, 0.25]
    want = {n: mix_restated([sd[n] for sd in sds], w32, sds[0][n].dtype) for n in ("a", "b")}
    assert torch.equal(model.a.data, want["a"]) and torch.equal(model.b.data, want["b"])
    stats = {"state": {"mean": [0.5], "std": [2.0]}}
    out = tmp_path / "mixed"
    path = cs.save_mixed(out, norm_stats=stats, as_float32=as_float32)
    assert path == str(out / "model.safetensors") and sorted(os.listdir(out)) == ["model.safetensors", "norm_stats.json"]
    back = load_file(path)
    assert set(back) == {"a", "b", "steps"} and int(back["steps"]) == 3
    assert back["a"].dtype == (F32 if as_float32 else BF16) and back["b"].dtype == F32
    assert torch.equal(back["a"].to(BF16), want["a"]) and torch.equal(back["b"], want["b"])
    assert json.loads((out / "norm_stats.json").read_text()) == {"norm_stats": stats}
    assert ma.load_norm_stats(out / "norm_stats.json") == stats


# ================================================================================================ keys
def test_tied_missing_and_gradient_less_parameters():
    """A tied parameter is mixed and projected once (also when the checkpoints hold it under its other name); a parameter the
    checkpoints lack is left alone and not projected; a parameter without a gradient is mixed but not projected."""
    model = Net()
    sds = [perturbed(model, k) for k in range(3)]
    for sd in sds:
        del sd["scale"]  # the checkpoints lack it
        del sd["embed"]  # the tied tensor only under its other name, as safetensors would have kept one of the two
    ops = TorchArithmeticOps()
    cs = ma.CheckpointSet(model, sds, ops=ops)
    assert cs.names == ["embed", "l1.weight", "l1.bias"] and cs.skipped == ["scale"]
    scale0 = model.scale.detach().clone()
    w = cs.mix_into([0.2, 0.5, 0.3])  # (returns the weights as it used them: rounded to f32)
    assert w == [float(np.float32(x)) for x in (0.2, 0.5, 0.3)]
    assert len(ops.mixes) == 3 and len(set(ops.mixes)) == 3
    assert torch.equal(model.scale, scale0)
    assert torch.equal(model.embed.data, mix_restated([sd["head.weight"] for sd in sds], w, F64)) and model.head.weight is model.embed
    model.l1.bias.requires_grad_(False)
    model.zero_grad()
    net_loss(model, batches()[0]).backward()
    assert model.scale.grad is not None and model.l1.bias.grad is None
    got = cs.project()
    assert len(ops.dots) == 2 and ops.dots == [model.embed.grad.data_ptr(), model.l1.weight.grad.data_ptr()]
    want = [float((model.embed.grad * sd["head.weight"]).sum() + (model.l1.weight.grad * sd["l1.weight"]).sum()) for sd in sds]
    assert got == pytest.approx(want, rel=1e-12)
    with pytest.raises(KeyError, match="l1.bias"):
        ma.CheckpointSet(model, [sds[0], {k: v for k, v in sds[1].items() if k != "l1.bias"}], ops=ops)
    with pytest.raises(ValueError, match="shape"):
        ma.CheckpointSet(model, [sds[0], {**sds[1], "l1.bias": torch.zeros(3, dtype=F64)}], ops=ops)


def test_more_than_eight_checkpoints():
    """project() calls the kernel in groups of at most 8 sources and still returns all N; mix_into refuses; a subset can be mixed."""
    model = Net()
    sds = [perturbed(model, k) for k in range(10)]
    ops = TorchArithmeticOps()
    cs = ma.CheckpointSet(model, sds, ops=ops)
    net_loss(model, batches()[0]).backward()
    got = cs.project()
    want = [float(sum((p.grad * sd[n]).sum() for n, p in model.named_parameters())) for sd in sds]
    assert len(got) == 10 and got == pytest.approx(want, rel=1e-12)
    assert ops.max_sources == 8 and len(ops.dots) == 2 * 4  # four parameters, two groups (8 + 2) each
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(ValueError, match="at most 8"):
        cs.mix_into([0.1] * 10)
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters())) and not ops.mixes
    cs.mix_into([0.25, 0.75], indices=[9, 2])  # weights follow their indices into source order
    assert torch.equal(model.l1.weight.data, mix_restated([sds[2]["l1.weight"], sds[9]["l1.weight"]], [0.75, 0.25], F64))
    for bad in ([0.5, 0.5, 0.5], [float("nan"), 1.0]):
        with pytest.raises(ValueError):
            cs.mix_into(bad, indices=[0, 1])


def test_mix_into_drops_the_inference_engine():
    class WithEngine(Point):
        dropped = 0

        def invalidate_inference_engine(self):
            self.dropped += 1

    model = WithEngine()
    ma.CheckpointSet(model, [{"theta": torch.ones(2, dtype=F64)}], ops=TorchArithmeticOps()).mix_into([1.0])
    assert model.dropped == 1 and torch.equal(model.theta.data, torch.ones(2, dtype=F64))


# ================================================================================================ header / binding
def test_entry_points_are_declared_and_bound():
    """The two prototypes are in include/kai0hip.h with the arguments _lib.py binds (test_cabi_v2_exports_every_declared_symbol then
    holds header and exports to the same set), and the hooks sit beside grad_accum_."""
    import ctypes as C

    from kai0_amd import _lib, optim

    header = open(os.path.join(ROOT, "include", "kai0hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int kai0_mix(const void* const* srcs, int src_f32, const float* weights, int n_src, void* dst, int dst_f32, int64_t n, "
            "kai0_stream_t stream);") in flat  # fmt: skip
    assert ("int kai0_multi_dot(const void* g, int g_f32, const void* const* srcs, int src_f32, int n_src, int64_t n, double* out, "
            "float* scratch, kai0_stream_t stream);") in flat  # fmt: skip
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib._PROTOS["kai0_mix"] == [C.POINTER(p), i, C.POINTER(C.c_float), i, p, i, i64, p]
    assert _lib._PROTOS["kai0_multi_dot"] == [p, i, C.POINTER(p), i, i, i64, p, p, p]
    assert {"kai0_mix", "kai0_multi_dot"} <= set(_lib.EXPORTED_SYMBOLS) and _lib.ABI_VERSION == 4
    assert callable(optim.mix_) and callable(optim.multi_dot_) and optim.MAX_MIX_SOURCES == ma.MAX_SOURCES == 8


def test_command_line_takes_the_reference_arguments():
    with pytest.raises(SystemExit):
        ma.main(["--help"])
    with pytest.raises(ValueError, match="Number of weights"):
        ma.main(["--config", "debug_pi05", "--data-path", "x.pkl", "--checkpoints", "a", "b", "--weights", "1.0", "--output", "o",
                 "--optimize_method", "greedy", "--num_iterations", "3", "--learning_rate", "0.1"])  # fmt: skip
