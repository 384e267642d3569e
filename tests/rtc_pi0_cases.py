"""The pi0 (`pi05=False`) cases of the real-time-chunking tests (tests/test_rtc_pi0_cpu.py, tests/test_rtc_pi0_gpu.py): builders only,
no HIP call.  A case is a CPU restatement pair (bf16 choreography, f32) on synthetic weights, a request and a previous chunk.

  tiny10 / tiny16 : tests/tiny.py's shapes with pi05=False at std 0.05, B = 2, Hs = 10 / 16 -> 11 / 17 suffix rows per sample (17: the
                    action key columns [P + 1, P + 17) cross an 8-column group of the probability rows behind the odd start);
  fullwidth       : tests/test_pi0_fullwidth_gpu.py's build (imported): the real widths at depth 2, B = 1, Hs = 50, P = 816, 867 keys.

The previous chunk is the batch's ground-truth actions on the 14 provided columns, as in tests/test_rtc_gpu.py (times PREV_SCALE)."""

import copy
import os

import torch

RTC = {"tiny10": dict(inference_delay=2, execute_horizon=6), "tiny16": dict(inference_delay=2, execute_horizon=6),
       "fullwidth": dict(inference_delay=3, execute_horizon=8)}  # fmt: skip
CAPS = (0.5, 2.5)
# The guided chunk must differ from the unguided one (tests/test_rtc_pi0_gpu.py asks >= 0.1 of the HIP engine; the f32 restatement
# itself must show >= 0.15, tests/test_rtc_pi0_cpu.py).  Measured on the f32 restatement, cap 0.5 / 2.5, with the ground-truth actions
# as the previous chunk: tiny10 0.193 / 0.490; tiny16 0.142 / 0.366; fullwidth 0.097 / 0.243.  The two cases that fall short take a
# scaled previous chunk instead: tiny16 1.5 x the actions (0.187 / 0.479), fullwidth 3 x (0.199 / 0.503; 2 x gives 0.146 / 0.366).
PREV_SCALE = {"tiny10": 1.0, "tiny16": 1.5, "fullwidth": 3.0}


def prev_of(actions):
    prev = torch.zeros_like(actions)
    prev[..., :14] = actions[..., :14]
    return prev


def f32_copy(restated):
    r32 = copy.deepcopy(restated)
    r32.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    return r32.eval()


def tiny_pi0(horizon: int = 10, std: float = 0.05, batch: int = 2):
    """-> dict(pcfg, ref, ref32, obs, actions, noise, prev): the tiny pi0 restatement pair and its request."""
    import dataclasses

    import pi0_restatement as R
    from tiny import tiny_cfgs

    from oracle.pi0_oracle import synthetic_batch

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    pcfg, ocfg05 = tiny_cfgs(action_horizon=horizon)
    blank = R.RestatedPI0(R.pi0_cfg(ocfg05))
    ref = R.build_restated(ocfg05, R.seeded_pi0_only(blank, seed=5, std=std), std)
    obs, actions, noise, _ = synthetic_batch(ref.config, batch, seed=0)
    return dict(pcfg=dataclasses.replace(pcfg, pi05=False, discrete_state_input=None), ref=ref, ref32=f32_copy(ref), obs=obs,
                actions=actions, noise=noise, prev=PREV_SCALE[f"tiny{horizon}"] * prev_of(actions))  # fmt: skip


def tiny_hip(case, device):
    """the HIP model carrying the case's weights"""
    from kai0_amd.model import PI0Pytorch

    model = PI0Pytorch(case["pcfg"])
    model.load_state_dict(case["ref"].state_dict(), strict=True)
    model.train_augmentation = False
    return model.to(device).eval()


def fullwidth_pi0():
    """-> dict(ref, ref32, obs, actions, noise, prev, cfg) at full width, depth 2, B = 1 (the builders of tests/test_pi0_fullwidth_gpu.py)."""
    from test_pi0_fullwidth_gpu import build_pi0_restated

    from oracle.pi0_oracle import synthetic_batch

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref, cfg = build_pi0_restated()
    obs, actions, noise, _ = synthetic_batch(cfg, 1, seed=3)
    return dict(ref=ref, ref32=f32_copy(ref), obs=obs, actions=actions, noise=noise, prev=PREV_SCALE["fullwidth"] * prev_of(actions), cfg=cfg)


def references(case, rtc_kw, *, delay: bool = False, steps=(0, 9)):
    """Everything the CPU computes for a case, once: the f32 unguided chunk, the f32 guided chunks at both caps with the trace of the
    default cap, the bf16 restatement's VJP at the f32 trace's first and last steps; with `delay` also the f32 chunk of
    `mask_prefix_delay=True` at the default cap."""
    import rtc_delay_restatement as D
    import rtc_restatement as R

    ref, r32, obs, noise = case["ref"], case["ref32"], case["obs"], case["noise"]
    for o in (ref, r32):
        o._state = obs.state
    kw = dict(prev_action_chunk=case["prev"], prefix_attention_schedule="exp", **rtc_kw)
    trace = []
    out = dict(plain=r32.sample_actions(obs, noise, num_steps=10), guided={0.5: R.sample_actions(r32, obs, noise, 10, trace=trace, **kw)},
               steps={})  # fmt: skip
    out["guided"][2.5] = R.sample_actions(r32, obs, noise, 10, max_guidance_weight=2.5, **kw)
    if delay:
        out["delay"] = D.sample_actions(r32, obs, noise, 10, mask_prefix_delay=True, **kw)
    ppad, cache = R.prefix_cache(ref, obs)
    for step in steps:
        x_t, t, _, e, corr32 = trace[step]
        _, _, _, corr_bf = R.x1_and_vjp(ref, ppad, cache, x_t, torch.tensor(t, dtype=torch.float32), lambda x1, e=e: e)
        out["steps"][step] = dict(x_t=x_t, t=t, e=e, corr32=corr32, corr_bf=corr_bf)
    return out
