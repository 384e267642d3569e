"""CPU restatement of the reference's real-time-chunking sampler WITH its `mask_prefix_delay` branch (`Pi0RTC.sample_actions`,
pi0_rtc.py:322-349), next to tests/rtc_restatement.py (imported, not edited: its `prefix_cache` / `velocity` / `x1_and_vjp` are the
blocks, and with the flag off this loop is that file's loop, statement for statement).

Read off the source:
    x_t_for_denoise = x_t                                                                         :322
    if mask_prefix_delay and provided_dim > 0:                                                    :323
        mask_time = arange(H) < d                                                                 :324
        x_t_for_denoise[..., :provided] = where(mask_time, prev[..., :provided], x_t[..., :provided])   :326-327
    x_1, vjp_fun, v_local = jax.vjp(denoiser, x_t_for_denoise)                                    :335   (v, x1, the Jacobian: at x_den)
    error = (prev - x_1) * weights * dim_mask;  pinv_correction = vjp_fun(error)                  :338-339
    v_t = nan_to_num(v_local - guidance_weight * pinv_correction);  return x_t + dt * v_t          :347-349  (the ORIGINAL x_t)

Both model families: `oracle` is an `OraclePI0` (pi0.5) or a `pi0_restatement.RestatedPI0`, whose `denoise_step` reads the state the
caller has set (`oracle._state = observation.state`; `sample_actions` here sets it)."""

import torch
from rtc_restatement import prefix_cache, x1_and_vjp

from kai0_amd import rtc


def linearisation_point(x_t, prev, d: int, provided: int):
    """:322-327 -> x_den = where(row < d and col < provided, prev, x_t) for [B, H, A] tensors."""
    H, A = x_t.shape[-2], x_t.shape[-1]
    mask = (torch.arange(H) < d)[None, :, None] & (torch.arange(A) < provided)[None, None, :]
    return torch.where(mask, prev, x_t)


def sample_actions(oracle, observation, noise, num_steps=10, *, prev_action_chunk=None, inference_delay=None, execute_horizon=None,
                   mask_prefix_delay=False, prefix_attention_schedule="exp", max_guidance_weight=0.5, enable_rtc=True, trace=None):  # fmt: skip
    """The guided Euler loop with the delay branch.  trace (a list): per step (x_t, t, v, e, corr, x_den) before the update."""
    cfg = oracle.config
    if hasattr(oracle, "_state"):
        oracle._state = observation.state
    ppad, cache = prefix_cache(oracle, observation)
    dt = torch.tensor(-1.0 / num_steps, dtype=torch.float32)
    x_t = noise
    time = torch.tensor(1.0, dtype=torch.float32)
    guided = enable_rtc and prev_action_chunk is not None
    if guided:
        gd = rtc.resolve(prev_action_chunk, batch=noise.shape[0], action_horizon=cfg.action_horizon, action_dim=cfg.action_dim,
                         inference_delay=inference_delay, execute_horizon=execute_horizon,
                         prefix_attention_schedule=prefix_attention_schedule, max_guidance_weight=max_guidance_weight)  # fmt: skip
        prev, w = torch.from_numpy(gd.prev), torch.from_numpy(gd.weights)
        mask = (torch.arange(cfg.action_dim) < gd.provided).to(torch.float32)
        d = max(0, min(int(inference_delay or 0), cfg.action_horizon))  # :301-302
    while time >= -dt / 2:
        if not guided:
            with torch.no_grad():
                v = oracle.denoise_step(ppad, cache, x_t, time.expand(noise.shape[0]))
            x_t = x_t + dt * v
        else:
            x_den = x_t
            if mask_prefix_delay and gd.provided > 0:
                x_den = linearisation_point(x_t, prev, d, gd.provided)
            v, _, e, corr = x1_and_vjp(oracle, ppad, cache, x_den, time, lambda x1: (prev - x1) * w[None, :, None] * mask)
            g = rtc.guidance_weight(float(time), max_guidance_weight)
            if trace is not None:
                trace.append((x_t.clone(), float(time), v.clone(), e.clone(), corr.clone(), x_den.clone()))
            v_new = torch.nan_to_num(v - g * corr, nan=0.0, posinf=0.0, neginf=0.0)
            x_t = x_t + dt * v_new
        time = time + dt
    return x_t
