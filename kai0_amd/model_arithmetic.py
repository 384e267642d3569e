"""Model arithmetic on the device: merge fine-tuned checkpoints that stay RESIDENT in HBM (model_arithmetic/arithmetic_torch.py,
model_arithmetic/common.py).

The reference's optimiser loop uploads every tensor of every checkpoint from numpy twice per iteration, mixes with N torch ops per
tensor, goes through `load_state_dict`, and takes the projection g_k = sum <param.grad, ckpt_k> with one `.item()` per tensor and
checkpoint.  Here the N checkpoints are loaded once, next to the model, in the parameters' own dtypes; an iteration is one `kai0_mix`
per parameter (straight into `p.data`), the forward / backward, one `kai0_multi_dot` per parameter, and ONE device-to-host copy.

    cs = CheckpointSet(model, [dir_a, dir_b, dir_c])
    w = optimize_gradient_descent(cs, batches, num_iterations=50, learning_rate=0.05)
    cs.mix_into(w, normalize=True)
    cs.save_mixed(out_dir, norm_stats=mix_norm_stats([...], w))

`python -m kai0_amd.model_arithmetic --config ... --data-path ... --checkpoints ... --output ...` takes arithmetic_torch.py's arguments.

Arithmetic (also DESIGN.md section 4): the merge accumulates `w0 x0 + w1 x1 + ...` in f32 in source order with one rounding to the
parameter's dtype, where the reference's final merge is a float64 `np.average`: at most about N f32 ulps before that rounding.
"""

from __future__ import annotations

import argparse
import json
import math
import os
import pathlib
import pickle

import numpy as np
import torch

MAX_SOURCES = 8  # what one kai0_mix / kai0_multi_dot launch takes


class HipArithmeticOps:
    """The two kernels via libkai0hip.so (kai0_amd.optim.mix_ / multi_dot_).  Any object with these two methods can be passed as
    `CheckpointSet(ops=...)`; the CPU tests pass torch stand-ins."""

    def mix(self, dst, srcs, weights):
        from .optim import mix_

        mix_(dst, srcs, weights)

    def multi_dot(self, grad, srcs, out):
        from .optim import multi_dot_

        multi_dot_(grad, srcs, out)


def resolve_torch_ckpt_path(path) -> str:
    """arithmetic_torch.py:49-57: the directory that holds model.safetensors, given that directory or its `params` child."""
    p = pathlib.Path(path).resolve()
    if (p / "model.safetensors").exists():
        return str(p)
    if p.name == "params" and (p.parent / "model.safetensors").exists():
        return str(p.parent)
    raise FileNotFoundError(f"Invalid PyTorch checkpoint path (no model.safetensors): {p}")


def _load_source(src) -> dict:
    if isinstance(src, (str, os.PathLike)):
        from safetensors.torch import load_file

        return load_file(os.path.join(resolve_torch_ckpt_path(src), "model.safetensors"))
    return src


class CheckpointSet:
    """N checkpoints resident beside `model`, ready to be mixed into it and to have its gradient projected onto them.

    sources: state dicts or checkpoint directories (`resolve_torch_ckpt_path`).  For every entry of `model.named_parameters()` — a
    tied parameter appears there once, so it is mixed and projected once, as in the reference's loop — the N source tensors are kept
    on the parameter's device in the parameter's own dtype and shape.  A parameter is looked up under its name, or, if it is tied and
    the files hold it under another of its names (safetensors keeps one name per tied group), under that one.  A parameter the FIRST
    checkpoint does not hold is left alone by `mix_into` and excluded from `project` (the reference's `strict=False` load and its
    `name in params_list[0]` test); one that a later checkpoint lacks is an error.
    More than 8 checkpoints: `project` calls the kernel in groups of 8 sources; `mix_into` raises (mixing in groups would add a
    rounding per group and break the stated arithmetic) — except that sources whose weight is not used at all can be left out with
    `indices=`, which is how `optimize_greedy` evaluates subsets.
    ops: the table of the two kernels (default: the HIP ones)."""

    def __init__(self, model, sources, *, ops=None):
        if len(sources) < 1:
            raise ValueError("CheckpointSet needs at least one checkpoint")
        self.model = model
        self.ops = ops if ops is not None else HipArithmeticOps()
        self.n = len(sources)
        aliases: dict[int, list[str]] = {}
        for name, p in model.state_dict(keep_vars=True).items():
            aliases.setdefault(id(p), []).append(name)
        self.names, self.params, self.sources, self.skipped = [], [], [], []
        entries = list(model.named_parameters())
        per_param: list[list] = [[] for _ in entries]
        keys: list[str | None] = []
        for k, src in enumerate(sources):  # one checkpoint on the host at a time
            sd = _load_source(src)
            if k == 0:
                for name, p in entries:
                    keys.append(next((a for a in [name, *aliases.get(id(p), [])] if a in sd), None))
            for (name, p), key, lst in zip(entries, keys, per_param):
                if key is None:
                    continue
                if key not in sd:
                    raise KeyError(f"checkpoint {k} has no tensor {key!r} (the first checkpoint has it)")
                t = sd[key]
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"checkpoint {k}: {key!r} has shape {tuple(t.shape)}, the model's parameter {tuple(p.shape)}")
                lst.append(t.detach().to(device=p.device, dtype=p.dtype, copy=True).contiguous())
            del sd
        for (name, p), key, lst in zip(entries, keys, per_param):
            if key is None:
                self.skipped.append(name)
                continue
            self.names.append(name)
            self.params.append(p)
            self.sources.append(lst)
        self._out = None

    # ---- mixing ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def mix_into(self, weights, *, normalize: bool = False, indices=None):
        """p.data = sum_k w_k * source_k for every covered parameter: one kai0_mix per parameter, f32 accumulation in source order,
        one rounding (module docstring).  Weights become f32 on the host; normalize=True first divides them by their sum in float64
        (common.mix_params).  indices: the sources the weights belong to (default all; at most 8).  These are raw writes behind
        autograd's version counters, so the model's inference engine is dropped."""
        given = list(range(self.n)) if indices is None else [int(i) for i in indices]
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != (len(given),):
            raise ValueError(f"{len(given)} checkpoints but weights of shape {w.shape}")
        if len(set(given)) != len(given) or not all(0 <= i < self.n for i in given):
            raise ValueError(f"indices must be distinct and in 0..{self.n - 1}, got {given}")
        order = sorted(range(len(given)), key=given.__getitem__)  # source order, whatever order the caller selected them in
        idx, w = [given[o] for o in order], w[order]
        if len(idx) > MAX_SOURCES:
            raise ValueError(f"mix_into takes at most {MAX_SOURCES} checkpoints in one merge, got {len(idx)}: mixing in groups would "
                             "round once per group; merge a subset (indices=) or merge hierarchically on purpose")  # fmt: skip
        if normalize:
            w = w / w.sum()
        if not np.all(np.isfinite(w)):
            raise ValueError(f"mixing weights must be finite, got {w.tolist()}")
        w32 = [float(x) for x in w.astype(np.float32)]
        for p, srcs in zip(self.params, self.sources):
            self.ops.mix(p.data, [srcs[i] for i in idx], w32)
        invalidate = getattr(self.model, "invalidate_inference_engine", None)
        if invalidate is not None:
            invalidate()
        return w32

    # ---- projection --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def project(self) -> list[float]:
        """g_k = sum over covered parameters with a gradient of <p.grad, source_k> (arithmetic_torch.py:206-214), as N floats: one
        zeroed f64 [N] device buffer, one kai0_multi_dot per parameter (and group of 8 sources), one device-to-host copy."""
        dev = self.params[0].device if self.params else torch.device("cpu")
        if self._out is None or self._out.device != dev:
            self._out = torch.zeros(self.n, dtype=torch.float64, device=dev)
        out = self._out
        out.zero_()
        for p, srcs in zip(self.params, self.sources):
            if p.grad is None:
                continue
            g = p.grad.detach().contiguous()
            for lo in range(0, self.n, MAX_SOURCES):
                self.ops.multi_dot(g, srcs[lo : lo + MAX_SOURCES], out[lo : lo + MAX_SOURCES])
        return out.cpu().tolist()

    # ---- writing -----------------------------------------------------------------------------------------------
    def save_mixed(self, output_dir, *, norm_stats: dict | None = None, as_float32: bool = False) -> str:
        """Writes the model as it stands (after `mix_into`) to <output_dir>/model.safetensors, and `norm_stats` (a plain dict as
        `mix_norm_stats` returns) to <output_dir>/norm_stats.json, where arithmetic_torch.py:554 puts it.  The default keeps the
        parameters' dtypes — what `create_trained_policy` here loads; as_float32=True writes float32 like `save_torch_params`
        (arithmetic_torch.py:72-83)."""
        from .checkpoint import save_model_safetensors

        os.makedirs(output_dir, exist_ok=True)
        path = os.path.join(output_dir, "model.safetensors")
        save_model_safetensors(self.model, path, dtype=torch.float32 if as_float32 else None)
        if norm_stats is not None:
            save_norm_stats(norm_stats, os.path.join(output_dir, "norm_stats.json"))
        return path


# ---------------------------------------------------------------------------------------------------- norm stats, weights
def load_norm_stats(path) -> dict:
    """common.py:22-28."""
    data = json.loads(pathlib.Path(path).read_text())
    if "norm_stats" not in data:
        raise ValueError(f"Invalid norm_stats format in {path}")
    return data["norm_stats"]


def save_norm_stats(norm_stats: dict, path) -> None:
    """common.py:55-60."""
    path = pathlib.Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps({"norm_stats": norm_stats}, indent=2))


def mix_norm_stats(norm_stats_list: list, weights=None) -> dict:
    """common.py:31-52: the weighted average (weights renormalised; equal if None) of every statistic of every dict-valued entry;
    entries that are not dicts are taken from the first."""
    if len(norm_stats_list) == 1:
        return norm_stats_list[0]
    if weights is None:
        weights = [1.0 / len(norm_stats_list)] * len(norm_stats_list)
    else:
        total = sum(weights)
        weights = [w / total for w in weights]
    result = {}
    for key, first in norm_stats_list[0].items():
        values = [ns[key] for ns in norm_stats_list]
        if isinstance(first, dict):
            result[key] = {stat: np.average(np.stack([np.array(v[stat]) for v in values], axis=0), axis=0, weights=weights).tolist()
                           for stat in first}  # fmt: skip
        else:
            result[key] = first
    return result


def inverse_loss_weights(losses) -> list[float]:
    """common.py:63-69: (1 / (loss + 1e-8))^2, normalised."""
    inv = (1.0 / (np.asarray(losses, dtype=np.float64) + 1e-8)) ** 2
    return (inv / inv.sum()).tolist()


# ---------------------------------------------------------------------------------------------------- losses
def default_loss(model, batch, noise=None, time=None):
    """The reference's objective: mean of the model's un-reduced flow-matching loss on (observation, actions)."""
    observation, actions = batch
    return model(observation, actions, noise=noise, time=time).mean()


def _pick(x, i: int):
    """noise= / time= may be None, one tensor for every batch, or one per batch."""
    if x is None or isinstance(x, torch.Tensor):
        return x
    return x[i]


def _mean_loss(cs: CheckpointSet, batches, loss_fn, noise, time) -> float:
    total = torch.zeros((), dtype=torch.float64)
    with torch.no_grad():
        for i, batch in enumerate(batches):
            total = total + loss_fn(cs.model, batch, noise=_pick(noise, i), time=_pick(time, i)).detach().double().cpu()
    return float(total) / len(batches)


def checkpoint_losses(cs: CheckpointSet, batches, *, loss_fn=default_loss, noise=None, time=None) -> list[float]:
    """Mean validation loss of every checkpoint on its own (arithmetic_torch.py:117-153): checkpoint k is copied into the model
    (a one-source mix with weight 1: exact) and evaluated under no_grad.  The model is left holding the last checkpoint."""
    losses = []
    for k in range(cs.n):
        cs.mix_into([1.0], indices=[k])
        losses.append(_mean_loss(cs, batches, loss_fn, noise, time))
    return losses


def projected_gradient(cs: CheckpointSet, weights, batch, *, adaptive: bool = False, loss_fn=default_loss, noise=None, time=None):
    """One iteration's device work (arithmetic_torch.py:188-218): mix the model with `weights` (a point of the simplex), back-propagate
    the loss of `batch`, project.  Returns (loss, g_k, d loss / d log-weights) with the last two as float64 tensors on the host:
    grad_log_w = w * (g_k - sum_j w_j g_j), times (loss / 0.05)^2 if adaptive (:311-313)."""
    w = torch.as_tensor(weights, dtype=torch.float64)
    cs.mix_into(w.tolist())
    loss = loss_fn(cs.model, batch, noise=noise, time=time)
    cs.model.zero_grad()
    loss.backward()
    g = torch.tensor(cs.project(), dtype=torch.float64)
    loss_val = float(loss.detach())
    grad = w * (g - (w * g).sum())
    if adaptive:
        grad = grad * (loss_val / 0.05) ** 2
    return loss_val, g, grad


def optimize_gradient_descent(cs: CheckpointSet, batches, *, num_iterations: int = 50, learning_rate: float = 0.1, adaptive: bool = False,
                              loss_fn=default_loss, noise=None, time=None, log=None, history=None) -> list[float]:  # fmt: skip
    """arithmetic_torch.py:156-246 (adaptive=True: :249-337).  Adam on log-weights (w = softmax), CosineAnnealingLR down to 1 % of the
    rate; iteration `it` takes `projected_gradient` on batch `it % len(batches)`.  Returns the weights of the iteration with the
    lowest loss.  The N log-weights and their optimiser live on the host in float64 (the reference keeps them in f32 on the device
    and reads them back every iteration).  history: a list that receives (loss, weights) of every iteration."""
    log_w = torch.zeros(cs.n, dtype=torch.float64, requires_grad=True)
    optimizer = torch.optim.Adam([log_w], lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=num_iterations, eta_min=learning_rate * 0.01)
    best_loss, best_w = math.inf, None
    for it in range(num_iterations):
        w = torch.softmax(log_w.detach(), dim=0)
        i = it % len(batches)
        loss_val, _, grad = projected_gradient(cs, w, batches[i], adaptive=adaptive, loss_fn=loss_fn, noise=_pick(noise, i),
                                               time=_pick(time, i))  # fmt: skip
        log_w.grad = grad
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        scheduler.step()
        if loss_val < best_loss:
            best_loss, best_w = loss_val, w.tolist()
        if history is not None:
            history.append((loss_val, w.tolist()))
        if log is not None:
            log(f"Iter {it + 1}/{num_iterations}: loss={loss_val:.6f}, weights={[round(x, 6) for x in w.tolist()]}")
    if log is not None:
        log(f"Best loss: {best_loss:.6f}, Best weights: {best_w}")
    return [float(x) for x in best_w]


def optimize_greedy(cs: CheckpointSet, batches, *, loss_fn=default_loss, noise=None, time=None, log=None) -> list[float]:
    """arithmetic_torch.py:340-427: start from the best single checkpoint, keep adding the checkpoint whose equal-weight merge with
    the selected ones lowers the mean validation loss most, stop when none does.  Weights: 1 / len(selected) on the selected."""

    def evaluate(indices) -> float:
        w = float(np.float32(1.0) / np.float32(len(indices)))  # the reference's float32 1 / n_sel
        cs.mix_into([w] * len(indices), indices=indices)
        return _mean_loss(cs, batches, loss_fn, noise, time)

    remaining, selected, best = list(range(cs.n)), [], math.inf
    for i in remaining:
        loss = evaluate([i])
        if log is not None:
            log(f"  Checkpoint {i + 1}: loss={loss:.6f}")
        if loss < best:
            best, selected = loss, [i]
    remaining.remove(selected[0])
    while remaining:
        round_best, candidate = best, -1
        for i in remaining:
            loss = evaluate([*selected, i])
            if log is not None:
                log(f"  {[s + 1 for s in selected]} + Checkpoint {i + 1}: loss={loss:.6f}")
            if loss < round_best:
                round_best, candidate = loss, i
        if candidate < 0:
            break
        best = round_best
        selected.append(candidate)
        remaining.remove(candidate)
    weights = [0.0] * cs.n
    for i in selected:
        weights[i] = 1.0 / len(selected)
    return weights


# ---------------------------------------------------------------------------------------------------- command line
def _to_batch(sample, device):
    """arithmetic_torch.py:87-101 + Observation.from_dict: a pickled (observation dict, actions) pair -> device tensors."""
    from .preprocessing import Observation

    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        return torch.from_numpy(np.asarray(v)).to(device)

    obs, actions = sample[0], sample[1]
    return Observation.from_dict({k: conv(v) for k, v in obs.items()}), conv(actions)


def _norm_stats_path(ckpt_dir: str) -> str | None:
    for d in (ckpt_dir, os.path.dirname(ckpt_dir.rstrip("/"))):
        if os.path.exists(os.path.join(d, "norm_stats.json")):
            return os.path.join(d, "norm_stats.json")
    return None


def main(argv=None) -> list[float]:
    """arithmetic_torch.py:455-568 with its arguments; returns the weights it merged with."""
    from . import normalize as _normalize
    from .policy import create_trained_policy
    from .training_config import get_config

    ap = argparse.ArgumentParser(description="Mix torch checkpoints (model.safetensors) on the device")
    ap.add_argument("--config", required=True, help="Config name")
    ap.add_argument("--data-path", required=True, help="Validation data pickle file: a list of (observation dict, actions)")
    ap.add_argument("--checkpoints", nargs="+", required=True, help="Checkpoint directories")
    ap.add_argument("--weights", nargs="+", type=float, help="Manual weights")
    ap.add_argument("--output", required=True, help="Output directory")
    ap.add_argument("--optimize_method", default="gradient_descent",
                    choices=["average", "inverse_loss", "gradient_descent", "adaptive_gradient_descent", "greedy"])  # fmt: skip
    ap.add_argument("--num_iterations", type=int, default=50)
    ap.add_argument("--learning_rate", type=float, default=0.05)
    ap.add_argument("--float32", action="store_true", help="write float32 tensors like the reference (default: the parameters' dtypes)")
    args = ap.parse_args(argv)
    if args.weights is not None and len(args.weights) != len(args.checkpoints):
        raise ValueError("Number of weights must match number of checkpoints")

    device = "cuda" if torch.cuda.is_available() else "cpu"
    config = get_config(args.config)
    with open(args.data_path, "rb") as f:
        samples = pickle.load(f)
    dirs = [resolve_torch_ckpt_path(p) for p in args.checkpoints]
    stats_path = _norm_stats_path(dirs[0])
    policy = create_trained_policy(config, dirs[0], pytorch_device=device,
                                   norm_stats=None if stats_path is None else _normalize.load(os.path.dirname(stats_path)))  # fmt: skip
    model = policy._model
    batches = [_to_batch(s, device) for s in samples]
    cs = CheckpointSet(model, dirs)

    losses = []
    weights = args.weights
    if weights is None:
        method = args.optimize_method
        if method == "average":
            weights = [1.0 / cs.n] * cs.n
        elif method in ("gradient_descent", "adaptive_gradient_descent"):
            weights = optimize_gradient_descent(cs, batches, num_iterations=args.num_iterations, learning_rate=args.learning_rate,
                                                adaptive=method == "adaptive_gradient_descent", log=print)  # fmt: skip
        elif method == "inverse_loss":
            losses = checkpoint_losses(cs, batches)
            weights = inverse_loss_weights(losses)
        else:
            weights = optimize_greedy(cs, batches, log=print)
        print(f"Optimized weights: {weights}")
    else:
        print(f"Using provided weights: {weights}")
        losses = checkpoint_losses(cs, batches)

    cs.mix_into(weights, normalize=True)
    stats_paths = [os.path.join(d, "norm_stats.json") for d in dirs]
    mixed_stats = None
    if all(os.path.exists(p) for p in stats_paths):
        mixed_stats = mix_norm_stats([load_norm_stats(p) for p in stats_paths], weights=list(weights))
    path = cs.save_mixed(args.output, norm_stats=mixed_stats, as_float32=args.float32)
    print(f"Saved mixed checkpoint to {path}")
    mixed_loss = _mean_loss(cs, batches, default_loss, None, None)
    print("Results:")
    for i, loss in enumerate(losses):
        print(f"  Ckpt {i + 1}: {loss:.6f} (w={weights[i]:.4f})")
    print(f"  Mixed:  {mixed_loss:.6f}")
    return [float(w) for w in weights]


if __name__ == "__main__":
    main()
