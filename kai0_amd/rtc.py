"""Real-time chunking (RTC): the host side of guided `sample_actions` (`src/openpi/models/pi0_rtc.py:47-61, 293-349`).

Every Euler step of a guided chunk is steered towards the not-yet-executed part of the previous chunk:
    v    = denoiser(x_t, t);   x1 = x_t - t v
    e    = (prev - x1) * w[row] * (col < provided)
    corr = (d x1 / d x_t)^T e = e - t (d v / d x_t)^T e
    v'   = nan_to_num(v - g corr);   x_t += dt v'
With `mask_prefix_delay` (:322-327) v, x1, e and the Jacobian are taken at x_den = x_t with the rows below the inference delay
overwritten by `prev` on the provided columns; the update still goes to x_t.
This module holds what is host arithmetic: the prefix weights `w`, the guidance weight `g` per step, and the handling of the request's
arguments.  The device side is `infer.InferenceEngine.sample_actions_guided` (the reverse sweep) and `csrc/rtc.hip` (the seams).
All of it is numpy float32: the values are launch constants and small static buffers of the engine.

The reference is JAX; these are restatements read off its source, not executed against it."""

from __future__ import annotations

import dataclasses

import numpy as np

SCHEDULES = ("ones", "zeros", "linear", "exp")
MAX_PROVIDED_DIM = 14  # pi0_rtc.py:320 — the two 7-DoF arms of the kai0 robots; dims past it are padding and are not steered


def get_prefix_weights(start: int, end: int, total: int, schedule: str) -> np.ndarray:
    """pi0_rtc.py:47-61 -> f32 [total].  Rows < start weigh 1 (the delay: they WILL be executed from the previous chunk), rows in
    [start, end) decay to 0 by `schedule`, rows >= end weigh 0."""
    if schedule not in SCHEDULES:
        raise ValueError(f"Invalid schedule: {schedule}")
    start = min(int(start), int(end))
    end = int(end)
    idx = np.arange(total, dtype=np.float32)
    if schedule == "ones":
        w = np.ones(total, dtype=np.float32)
    elif schedule == "zeros":
        w = (idx < start).astype(np.float32)
    else:
        w = np.clip((np.float32(start - 1) - idx) / np.float32(end - start + 1) + np.float32(1), 0, 1).astype(np.float32)
        if schedule == "exp":
            w = (w * np.expm1(w) / np.float32(np.e - 1)).astype(np.float32)
    return np.where(idx >= end, np.float32(0), w).astype(np.float32)


def guidance_weight(t: float, max_guidance_weight: float) -> float:
    """pi0_rtc.py:340-346: tau = clip(1 - t, 1e-3, 1);  g = min((1 - tau) / tau * ((1 - tau)^2 + tau^2) / (1 - tau)^2, cap), in f32.
    (1 - tau = 0 at t = 0 is never visited: the schedule's last time is 1 / num_steps.)"""
    tau = np.clip(np.float32(1.0) - np.float32(t), np.float32(1e-3), np.float32(1.0))
    om = np.float32(1.0) - tau
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_r2 = (om * om + tau * tau) / (om * om)
        c = om / tau
        g = c * inv_r2
    if not np.isfinite(g):  # nan_to_num(c, posinf=cap) and min(.., cap) of the reference
        g = np.float32(max_guidance_weight)
    return float(np.minimum(np.float32(g), np.float32(max_guidance_weight)))


def guidance_weights(times, max_guidance_weight: float) -> list[float]:
    return [guidance_weight(t, max_guidance_weight) for t in times]


@dataclasses.dataclass
class Guidance:
    """A guided call's arguments, resolved: prev f32 [B, H, A] (finite, padded / cut to A), w f32 [H], provided (columns steered);
    mask_prefix_delay with delay_rows f32 [H] = (row < inference delay) ? 1 : 0, the rows it overwrites (:324)."""

    prev: np.ndarray
    weights: np.ndarray
    provided: int
    max_guidance_weight: float
    mask_prefix_delay: bool = False
    delay_rows: np.ndarray | None = None


def resolve(prev_action_chunk, *, batch: int, action_horizon: int, action_dim: int, inference_delay=None, execute_horizon=None,
            prefix_attention_schedule: str = "exp", max_guidance_weight: float = 0.5, mask_prefix_delay: bool = False) -> Guidance:  # fmt: skip
    """pi0_rtc.py:299-324, 337 for a previous chunk [H, A'] or [B, H, A'] (array, tensor or nested lists)."""
    if prefix_attention_schedule not in SCHEDULES:
        raise ValueError(f"Invalid schedule: {prefix_attention_schedule}")
    if hasattr(prev_action_chunk, "detach"):
        prev_action_chunk = prev_action_chunk.detach().cpu().numpy()
    prev = np.asarray(prev_action_chunk, dtype=np.float32)
    if prev.ndim == 2:
        prev = prev[None, ...]
    if prev.ndim != 3:
        raise ValueError(f"prev_action_chunk must be [H, A'] or [B, H, A'], got shape {prev.shape}")
    H = action_horizon
    if prev.shape[1] != H:
        raise ValueError(f"prev_action_chunk has {prev.shape[1]} rows, the model's action_horizon is {H}")
    if prev.shape[0] not in (1, batch):
        raise ValueError(f"prev_action_chunk has batch {prev.shape[0]}, the request has {batch}")
    exec_h = int(np.clip(H if execute_horizon is None or execute_horizon == 0 else int(execute_horizon), 1, H))
    d = int(np.clip(0 if inference_delay is None else int(inference_delay), 0, H))
    a_given = prev.shape[2]
    prev = np.nan_to_num(prev, nan=0.0, posinf=0.0, neginf=0.0)
    if a_given > action_dim:
        prev = prev[..., :action_dim]
    elif a_given < action_dim:
        prev = np.concatenate([prev, np.zeros((*prev.shape[:2], action_dim - a_given), dtype=np.float32)], axis=-1)
    prev = np.array(np.broadcast_to(prev, (batch, H, action_dim)), dtype=np.float32)  # (a writable copy)
    return Guidance(prev=prev, weights=get_prefix_weights(d, exec_h, H, prefix_attention_schedule),
                    provided=min(MAX_PROVIDED_DIM, a_given, action_dim), max_guidance_weight=float(max_guidance_weight),
                    mask_prefix_delay=bool(mask_prefix_delay), delay_rows=(np.arange(H) < d).astype(np.float32))  # fmt: skip
