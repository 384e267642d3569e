"""CPU restatement of the reference's real-time-chunking sampler (`Pi0RTC.sample_actions`, pi0_rtc.py:233-360), assembled from the blocks
of `oracle.pi0_oracle` (imported, not edited): the oracle's `embed_prefix`, its prefix forward into the KV cache and its
`denoise_step` as the denoiser, `torch.autograd.grad(x1, x_t, e)` as `jax.vjp`, in whatever precision the oracle's weights are in
(f32: the arbiter; bf16: the rounding choreography the HIP engine follows, whose distance from f32 sizes the engine's bounds).

The reference is JAX and cannot be executed next to this suite: the loop below is read off its source, step for step
(rtc_step :293-349, get_prefix_weights :47-61, which is restated once, in kai0_amd.rtc).  tests/test_rtc_cpu.py pins the host
arithmetic to hand-computed values, this loop with no previous chunk to `oracle.sample_actions`, and its VJP to a finite difference
of the float64 oracle."""

import torch

from kai0_amd import rtc


def prefix_cache(oracle, observation):
    """pi0_pytorch.py:381-393: the prefix pass -> (prefix pad masks, per-layer (k, v))."""
    from oracle import pi0_oracle as O

    images, img_masks, lang_tokens, lang_masks = oracle._unpack(observation)
    with torch.no_grad():
        pe, ppad, patt = oracle.embed_prefix(images, img_masks, lang_tokens, lang_masks)
        p2d = O.make_att_2d_masks(ppad, patt)
        ppos = torch.cumsum(ppad, dim=1) - 1
        _, cache = oracle.paligemma_with_expert.forward(
            attention_mask=O.masks_4d(p2d), position_ids=ppos, past_key_values=None, inputs_embeds=[pe, None], use_cache=True
        )
    return ppad, cache


def velocity(oracle, ppad, cache, x_t, t):
    """v = denoiser(x_t, t): the oracle's `denoise_step`.  (float64 weights, the finite-difference check: the same body with the
    output slice cast to the head's dtype instead of `denoise_step`'s hard-coded float32.)"""
    from oracle import pi0_oracle as O

    b = x_t.shape[0]
    ts = t.expand(b)
    if oracle.action_out_proj.weight.dtype != torch.float64:
        return oracle.denoise_step(ppad, cache, x_t, ts)
    se, spad, satt, cond = oracle.embed_suffix(x_t, ts)
    plen, slen = ppad.shape[1], spad.shape[1]
    full = torch.cat([ppad[:, None, :].expand(b, slen, plen), O.make_att_2d_masks(spad, satt)], dim=2)
    position_ids = torch.sum(ppad, dim=-1)[:, None] + torch.cumsum(spad, dim=1) - 1
    outs, _ = oracle.paligemma_with_expert.forward(
        attention_mask=O.masks_4d(full), position_ids=position_ids, past_key_values=cache, inputs_embeds=[None, se], use_cache=False,
        adarms_cond=[None, cond],
    )  # fmt: skip
    return oracle.action_out_proj(outs[1][:, -oracle.config.action_horizon :].to(torch.float64))


def x1_and_vjp(oracle, ppad, cache, x_t, t, cotangent):
    """(v, x1 = x_t - t v, e, (d x1 / d x_t)^T e) at x_t (pi0_rtc.py:329-339); e = cotangent(x1), a tensor function of the detached x1."""
    x_in = x_t.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        v = velocity(oracle, ppad, cache, x_in, t)
        x1 = x_in - t * v
        e = cotangent(x1.detach())
        corr = torch.autograd.grad(x1, x_in, e)[0]
    return v.detach(), x1.detach(), e, corr


def sample_actions(oracle, observation, noise, num_steps=10, *, prev_action_chunk=None, inference_delay=None, execute_horizon=None,
                   prefix_attention_schedule="exp", max_guidance_weight=0.5, enable_rtc=True, trace=None):  # fmt: skip
    """The guided Euler loop.  trace (a list): per step (x_t, t, v, e, corr) before the update."""
    cfg = oracle.config
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
    while time >= -dt / 2:
        if not guided:
            with torch.no_grad():
                v = oracle.denoise_step(ppad, cache, x_t, time.expand(noise.shape[0]))
            x_t = x_t + dt * v
        else:
            v, _, e, corr = x1_and_vjp(oracle, ppad, cache, x_t, time, lambda x1: (prev - x1) * w[None, :, None] * mask)
            g = rtc.guidance_weight(float(time), max_guidance_weight)
            if trace is not None:
                trace.append((x_t.clone(), float(time), v.clone(), e.clone(), corr.clone()))
            v_new = torch.nan_to_num(v - g * corr, nan=0.0, posinf=0.0, neginf=0.0)
            x_t = x_t + dt * v_new
        time = time + dt
    return x_t
