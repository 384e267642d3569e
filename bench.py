"""bench.py — pi0.5 full fine-tune throughput (train samples/s) on N MI355X, plus p50 action-chunk latency.

Contract (see the round prompt): `python bench.py --gpus N --steps K --warmup W`; for N>1 the driver launches it
under torch.distributed.run, one rank per GPU over RCCL.  Rank 0 prints ONE JSON line.

Workload (BASELINE.json configs[1]): pi0.5 full fine-tune, bf16 compute, batch 32 per GPU, 3 cameras 224x224 +
200 prompt tokens + 50x32 action chunk, synthetic data resident in HBM, random-init weights of the real
architecture (3.617 B stored / 3.353 B used parameters).  A step = augmentation + forward + backward + global-norm
clip + fused AdamW over every parameter: nothing that contributes to the loss, a gradient or an update is skipped inside the
timed region (the last layer's prefix o_proj + MLP, whose output nothing reads, are dead values and not computed — see
TRAIN_TFLOP_NEEDED_PER_SAMPLE).

A plain run sets up, warms up, times the steps and prints the line (`ms_per_step` = one timed step).  `--dump-outputs DIR`
writes what the last timed step computed to DIR/*.npy (float32, see `dump_outputs`); the inputs and weights are seeded, so two
builds run with the same arguments can be compared array by array.

Extra objects on the same line, measured only with `--full` (each takes runs of its own after the timed region):
  ranks        — who took part: world size, device identities, per-rank step time (N > 1: also `comm`, the other partition).
  trimmed_prompt — the same step with the prompt cut to the longest valid prompt of the batch (model.trim_prompt_padding).
  roofline     — the dominant kernel (gemm_bf16_kernel): achieved = algorithmic FLOPs (2 M N K of every launch; SURVEY.md
                 §8d: 14.04 TFLOP per sample per train step) / summed GEMM launch durations, measured with HIP events on
                 the launch stream over two further identical steps run right after the timed region (inside it the event
                 records cost ~10 ms per step); peak = 2.5 PFLOP/s dense bf16 MFMA.
  inference    — p50 of one B = 1 action chunk (SigLIP + prefix pass + 10 Euler steps, hipGraph replay, chunk copied to the
                 host), its three stage times, and the chunk against its floors: 5.02 TFLOP of MFMA work and 9.0 GB of
                 weight traffic.
  cpu_baseline — the CPU oracle (a port: the reference cannot be imported here) timed on the host cores on the REAL
                 network (all 18 joint + 27 SigLIP layers, full widths): one sample forward + backward, plus clip + AdamW
                 over every parameter; see `sample`.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

# RCCL / device-tensor sharing across processes on this driver needs dmabuf IPC; must be in the environment before HIP initialises
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TRAIN_TFLOP_PER_SAMPLE = 14.04  # 3 x 4.68 TFLOP forward, no remat, no unused lm_head
# ... of which 3 x 0.203 TFLOP are the LAST layer's prefix o_proj + MLP, whose output nothing reads (the model's output is the
# suffix): dead values that the reference's jitted JAX step never computes (XLA removes them), whose backward never existed
# under autograd either, and that model.forward_joint skips.  The step fraction below is priced on what is needed, 13.43.
TRAIN_TFLOP_NEEDED_PER_SAMPLE = 14.04 - 3 * (2 * 968 * 2048 * 2048 + 3 * 2 * 968 * 2048 * 16384) / 1e12
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA


def synthetic_batch(cfg, batch: int, seed: int, device):
    """SURVEY.md §8d synthetic inputs, generated on the device."""
    from kai0_amd.preprocessing import IMAGE_KEYS, Observation

    g = torch.Generator(device=device).manual_seed(seed)
    hw = cfg.siglip.image_size
    images, masks = {}, {}
    for k in IMAGE_KEYS:
        u8 = torch.randint(0, 256, (batch, hw, hw, 3), generator=g, device=device, dtype=torch.uint8)
        images[k] = (u8.to(torch.float32) / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()
        masks[k] = torch.ones(batch, dtype=torch.bool, device=device)
    L = cfg.max_token_len
    tokens = torch.randint(0, 2048, (batch, L), generator=g, device=device, dtype=torch.int64)
    n_valid = 64 + torch.randint(0, 65, (batch,), generator=g, device=device)
    tmask = torch.arange(L, device=device)[None, :] < n_valid[:, None]
    state = torch.zeros(batch, cfg.action_dim, device=device)
    state[:, :14] = torch.rand(batch, 14, generator=g, device=device) * 2 - 1
    actions = torch.zeros(batch, cfg.action_horizon, cfg.action_dim, device=device)
    actions[..., :14] = torch.randn(batch, cfg.action_horizon, 14, generator=g, device=device)
    obs = Observation(images=images, image_masks=masks, state=state, tokenized_prompt=tokens, tokenized_prompt_mask=tmask)
    return obs, actions


def build_model(cfg, device, seed: int):
    from kai0_amd.model import PI0Pytorch

    torch.manual_seed(seed)
    with torch.device(device):
        model = PI0Pytorch(cfg)
    # explicit weights — plain RMSNorm weights 0 (checkpoint-like), adaRMS dense non-trivial
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "dense.weight" in name:
                p.normal_(0.0, 0.02)
    return model


class GemmTimer:
    """Brackets every kai0_gemm_bf16 launch — and every attention-kernel launch (`_lib.call` of the attention entry points) — with
    HIP events on the launch stream (torch's current stream)."""

    ATTN_ENTRY = {"kai0_attn_fwd": "joint_attention_kernels", "kai0_attn_bwd_dq2": "joint_attention_kernels",
                  "kai0_attn_bwd_dq": "joint_attention_kernels", "kai0_siglip_attn_fwd": "siglip_attention_kernels",
                  "kai0_siglip_attn_bwd2": "siglip_attention_kernels", "kai0_siglip_attn_bwd": "siglip_attention_kernels"}  # fmt: skip

    def __init__(self):
        self.events = []
        self.kernel_events = []

    def install(self):
        from kai0_amd import _lib, ops

        self._orig = ops.gemm
        self._orig_call = _lib.call
        timer = self

        def timed_gemm(A, B, out, **kw):
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            r = timer._orig(A, B, out, **kw)
            e.record()
            # act 6 (gate | up pair GEMM): N names the MLP width, the launch multiplies by both weights
            timer.events.append((s, e, 2.0 * kw["M"] * kw["N"] * kw["K"] * kw.get("batch", 1) * (2 if kw.get("act", 0) == 6 else 1),
                                 (int(kw.get("a_kc", True)), int(kw.get("b_kc", True)), kw["M"], kw["N"], kw["K"], kw.get("batch", 1))))
            return r

        def timed_call(name, *args):
            fam = timer.ATTN_ENTRY.get(name)
            if fam is None:
                return timer._orig_call(name, *args)
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            r = timer._orig_call(name, *args)
            e.record()
            timer.kernel_events.append((s, e, fam))
            return r

        ops.gemm = timed_gemm
        _lib.call = timed_call

    def uninstall(self):
        from kai0_amd import _lib, ops

        ops.gemm = self._orig
        _lib.call = self._orig_call

    def summarize(self):
        ms = sum(s.elapsed_time(e) for s, e, _, _ in self.events)
        fl = sum(f for _, _, f, _ in self.events)
        return ms, fl, len(self.events)

    def breakdown(self):
        agg = {}
        for s, e, f, key in self.events:
            a = agg.setdefault(key, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += s.elapsed_time(e)
            a[2] += f
        rows = sorted(agg.items(), key=lambda kv: -kv[1][1])
        return [{"a_kc": k[0], "b_kc": k[1], "M": k[2], "N": k[3], "K": k[4], "batch": k[5], "calls": v[0], "ms": v[1],
                 "tflops": v[2] / v[1] / 1e9} for k, v in rows]

    def families(self, batch: int, steps: int):
        """The bf16 GEMM launches by the family north_star's targets are written in (">= 40 % MFMA on Gemma / ViT blocks"), from the
        launch shapes: M (or, for the transposed-operand weight gradients, K) = batch x 968 prefix rows -> Gemma-2B; batch x 768
        patch rows -> SigLIP (its projector included); batch x 50 action rows -> the 300M expert; batched launches -> the dV | dK
        GEMM of the joint attention backward.  Per family: ms and TFLOP per step, achieved TFLOP/s, fraction of the 2.5 PFLOP/s
        peak.  `attention` = the attention kernels' launches (kai0_attn_fwd / kai0_attn_bwd_dq2 / kai0_siglip_attn_*) + that dV | dK
        GEMM, priced on the ALGORITHMIC attention work (4 Sq Sk heads hd per layer forward, twice that backward — the
        recomputed logits of the backward kernel are not credited)."""
        rows_gemma, rows_siglip, rows_expert = batch * 968, batch * 768, batch * 50
        fam = {}

        def add(name, ms, fl):
            a = fam.setdefault(name, [0.0, 0.0, 0])
            a[0] += ms
            a[1] += fl
            a[2] += 1

        for s, e, f, (a_kc, b_kc, M, N, K, nb) in self.events:
            ms = s.elapsed_time(e)
            wgrad = not a_kc and not b_kc
            rows = K if wgrad else M
            if nb > 1:
                add("attention_dv_dk_gemm", ms, f)
            elif rows == rows_gemma:
                add("gemma_wgrad" if wgrad else "gemma_linear", ms, f)
            elif rows == rows_siglip:
                add("siglip_wgrad" if wgrad else "siglip_linear", ms, f)
            elif rows == rows_expert:
                add("expert_wgrad" if wgrad else "expert_linear", ms, f)
            else:
                add("other", ms, f)
        for s, e, name in self.kernel_events:
            add(name, s.elapsed_time(e), 0.0)
        out = {}
        for k, (ms, fl, n) in fam.items():
            out[k] = {"ms_per_step": ms / steps, "launches_per_step": n // steps}
            if fl > 0:
                out[k].update({"tflop_per_step": fl / steps / 1e12, "tflops": fl / 1e9 / ms, "frac": fl / 1e9 / ms / MFMA_BF16_PEAK_TFLOPS})
        for grp, parts in (("gemma_blocks", ("gemma_linear", "gemma_wgrad")), ("vit_blocks", ("siglip_linear", "siglip_wgrad"))):
            ms = sum(fam[p][0] for p in parts if p in fam)
            fl = sum(fam[p][1] for p in parts if p in fam)
            if ms > 0:
                out[grp] = {"ms_per_step": ms / steps, "tflop_per_step": fl / steps / 1e12, "tflops": fl / 1e9 / ms,
                            "frac": fl / 1e9 / ms / MFMA_BF16_PEAK_TFLOPS, "members": list(parts)}
        # attention: kernels + the dV | dK GEMM, priced on algorithmic work
        att_ms = sum(fam[k][0] for k in ("joint_attention_kernels", "attention_dv_dk_gemm") if k in fam)
        if att_ms > 0:
            alg = 3 * 4 * 1018 * 1018 * 2048 * 18 * batch  # forward + 2x backward, 18 layers, per step
            out["attention"] = {"ms_per_step": att_ms / steps, "algorithmic_tflop_per_step": alg / 1e12, "tflops": alg * steps / 1e9 / att_ms,
                                "frac": alg * steps / 1e9 / att_ms / MFMA_BF16_PEAK_TFLOPS,
                                "members": ["joint_attention_kernels", "attention_dv_dk_gemm"],
                                "note": "algorithmic 4 Sq Sk (heads hd) per layer forward, 8 backward; the backward kernel's recomputed logits are not credited"}
        if "siglip_attention_kernels" in fam:
            alg = 3 * 4 * 256 * 256 * 1152 * 27 * 3 * batch
            ms = fam["siglip_attention_kernels"][0]
            out["siglip_attention_kernels"].update({"algorithmic_tflop_per_step": alg / 1e12, "tflops": alg * steps / 1e9 / ms,
                                                    "frac": alg * steps / 1e9 / ms / MFMA_BF16_PEAK_TFLOPS})
        return out


def _oracle_full_depth(O, vocab: int):
    """The full-depth, full-width oracle (fp32), built without the minutes of nn.init / seeded randn a multi-billion-parameter CPU
    model costs: allocated on the meta device, materialised, and filled from one N(0, 0.02) block tiled over every matrix
    (values only need to be of the right scale for a timing).  `vocab`: 257152 (the benchmarked model: the embedding table's 0.53 B
    parameters take part in clip + AdamW) when the host has the memory, else 2048 (the table carries no FLOPs)."""
    cfg = O.OracleConfig(dtype="float32", vocab_size=vocab)
    with torch.device("meta"):
        model = O.OraclePI0(cfg)
    model.to_empty(device="cpu")
    block = torch.randn(1 << 22, generator=torch.Generator().manual_seed(0)) * 0.02
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 and "norm" in n and "dense" not in n:
                p.fill_(1.0 if "vision" in n else 0.0)  # LayerNorm weight 1 / bias below; plain RMSNorm weight 0 (checkpoint-like)
            else:
                flat = p.view(-1)
                for lo in range(0, flat.numel(), block.numel()):
                    hi = min(flat.numel(), lo + block.numel())
                    flat[lo:hi].copy_(block[: hi - lo])
        for mod in model.modules():  # non-persistent buffers are not materialised by to_empty
            if isinstance(getattr(mod, "inv_freq", None), torch.Tensor):
                mod.inv_freq = O.rope_inv_freq(mod.inv_freq.numel() * 2)
            if isinstance(mod, O.SiglipVisionEmbeddings):
                mod.position_ids = torch.arange(mod.num_patches).expand((1, -1))
    return model, cfg


def cpu_baseline(batch: int = 32):
    """The CPU oracle (kind "port": the reference cannot be imported in this image) timed on the host cores on the REAL
    network: one sample through forward + backward of all 27 SigLIP x 3 cameras and 18 joint Gemma-2B / expert layers in fp32
    (bf16 matmuls are emulated on hosts without AMX and would understate the CPU), then `clip_grad_norm_` + `AdamW.step()`
    (the reference trainer's calls, train_pytorch.py:557-561) over every parameter.  A training step of the benchmarked
    workload (batch 32) = 32 x the per-sample forward/backward + one optimizer pass: value = 32 / (32 t_fb + t_opt).
    Bounded: one warm pass + one timed pass (~10-25 s each on a 64-core host); nothing is extrapolated across layers."""
    import psutil

    from oracle import pi0_oracle as O

    # the cores this process may use (affinity / OMP_NUM_THREADS), not the machine's count: more threads than cores only slow it down
    cores = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS") or 64), 64)
    torch.set_num_threads(cores)
    t0 = time.time()
    # full vocabulary if the host has room: 4.14 B stored f32 parameters + gradients + two AdamW moments of the 3.35 B
    # trained ones ~ 16.6 + 13.4 + 26.8 GB; otherwise the 2048-row table of the earlier rounds (stated in `vocab`)
    vocab = 257152 if psutil.virtual_memory().available > (96 << 30) else 2048
    model, cfg = _oracle_full_depth(O, vocab)
    init_s = time.time() - t0
    obs, actions, noise, t = O.synthetic_batch(cfg, 1, seed=0)
    times = []
    for _ in range(2):  # the first pass also pages the 11 GB of weights in
        model.zero_grad(set_to_none=True)
        t0 = time.time()
        model(obs, actions, noise, t).mean().backward()
        times.append(time.time() - t0)
        if times[-1] > 45.0:
            break
    t_fb = min(times)
    # optimizer: every parameter that received a gradient, if the host has room for the two moment buffers (8 B/param);
    # otherwise the expert tower + SigLIP only, scaled by parameter count (the update is linear in it)
    params = [p for p in model.parameters() if p.grad is not None]
    n_all = sum(p.numel() for p in params)
    subset = params
    if psutil.virtual_memory().available < 12 * n_all + (16 << 30):
        subset = [p for n, p in model.named_parameters() if p.grad is not None and "language_model" not in n]
    n_sub = sum(p.numel() for p in subset)
    opt = torch.optim.AdamW(subset, lr=2.5e-5, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-10, foreach=False)
    t0 = time.time()
    torch.nn.utils.clip_grad_norm_(subset, 1.0, foreach=False)
    opt.step()
    t_opt = (time.time() - t0) * n_all / n_sub
    step_s = batch * t_fb + t_opt
    # the action chunk on the same host cores: oracle `sample_actions`, B = 1, prefix pass with KV cache + 10
    # Euler steps, fp32, no autograd; one timed call (the forward/backward passes above already paged the weights in)
    del opt
    model.zero_grad(set_to_none=True)
    noise1 = torch.randn(1, cfg.action_horizon, cfg.action_dim, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        t0 = time.time()
        model.sample_actions(obs, noise1, num_steps=10)
        t_chunk = time.time() - t0
    infer = {"value": t_chunk * 1e3, "unit": "ms per action chunk (B = 1, 10 steps)", "cores": cores, "kind": "port",
             "sample": f"fp32 oracle `sample_actions` at full depth and width, one call after the weights were paged in: {t_chunk:.2f} s"}  # fmt: skip
    return {
        "inference": infer,
        "value": batch / step_s,
        "unit": "samples/s",
        "cores": cores,
        "kind": "port",
        "vocab": int(cfg.vocab_size),
        "vocab_note": ("full vocabulary: the 257152-row embedding table's gradient, clip and AdamW update (0.53 B of the 3.35 B trained parameters) are "
                       "in fwd_bwd_s_per_sample / optimizer_s" if vocab == 257152 else
                       "the oracle is timed at vocab 2048 (host memory): the 257152-row embedding table carries no FLOPs; its AdamW update "
                       "(0.53 B of the 3.35 B trained parameters) is NOT in optimizer_s"),
        "fwd_bwd_s_per_sample": t_fb,
        "optimizer_s": t_opt,
        "init_s": init_s,
        "sample": f"fp32 oracle, full depth and width (18 joint + 27 SigLIP layers x 3 cameras, {n_all / 1e9:.2f} B parameters with "
        f"gradients; vocab {vocab}): 1 sample forward+backward = {t_fb:.2f} s (best of {len(times)}: "
        f"{', '.join(f'{x:.1f}' for x in times)}), clip_grad_norm_ + AdamW.step over "
        f"{'all' if n_sub == n_all else f'{n_sub / 1e9:.2f} B (scaled by count to all)'} parameters = {t_opt:.2f} s; "
        f"a batch-{batch} step = {batch} x {t_fb:.2f} + {t_opt:.2f} = {step_s:.1f} s; model construction {init_s:.1f} s not included",
    }


INFER_TFLOP = 5.02  # prefix pass 4.635 TFLOP + 10 x 38.9 GFLOP
INFER_GB = 9.0      # 4.79 GB prefix weights + 10 x 0.42 GB expert weights (bf16, modulations precomputed)
HBM_PEAK_TBS = 8.0  # MI355X_MICROARCH.md: HBM3E spec


def _graph_time_ms(fn, iters: int = 20):
    """p50 wall time of `fn` replayed from its own hipGraph (device time: events on the replay stream)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2]


def measure_latency(model, cfg, device, iters: int = 40):
    """One B = 1 action chunk (prefix pass + 10 denoise steps, hipGraph): p50 of the Policy-level model time (replay + the
    chunk's copy to the host, policy.py:114-118), and the three stages timed as graphs of their own."""
    model.eval()
    obs, _ = synthetic_batch(cfg, 1, seed=123, device=device)
    noise = torch.randn(1, cfg.action_horizon, cfg.action_dim, device=device)
    for _ in range(3):
        model.sample_actions(device, obs, noise=noise, num_steps=10)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = model.sample_actions(device, obs, noise=noise, num_steps=10)
        out.cpu()  # Policy.infer moves the chunk to the host (policy.py:114-118)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    p50 = ts[len(ts) // 2]
    res = {"p50_ms": p50, "min_ms": ts[0], "p90_ms": ts[int(len(ts) * 0.9)]}
    try:
        eng = model._engine
        si = eng._static_in
        with torch.no_grad():
            t_sig = _graph_time_ms(lambda: eng._siglip(torch.cat(si["images"], dim=0)))
            t_pre = _graph_time_ms(lambda: eng._prefix_pass(si["images"], si["img_masks"], si["lang_tokens"], si["lang_masks"]))
            t_all = _graph_time_ms(lambda: eng._run(si["images"], si["img_masks"], si["lang_tokens"], si["lang_masks"], si["noise"], 10))
        res["stages_ms"] = {"siglip": t_sig, "prefix": t_pre - t_sig, "denoise_10_steps": t_all - t_pre, "graph_total": t_all}
    except Exception as e:  # noqa: BLE001 - the stage split is diagnostics; the p50 above stands on its own
        res["stages_error"] = repr(e)[:200]
    # Extra (not the headline p50): the serve path's default — the prompt slots the request does not fill are not computed
    # (model.trim_prompt_padding_infer, policy.create_trained_policy).  The p50 above computes all 200 slots, as the reference does.
    try:
        model.trim_prompt_padding_infer = True
        for _ in range(3):
            model.sample_actions(device, obs, noise=noise, num_steps=10)
        torch.cuda.synchronize()
        tt = []
        for _ in range(iters):
            t0 = time.perf_counter()
            model.sample_actions(device, obs, noise=noise, num_steps=10).cpu()
            tt.append((time.perf_counter() - t0) * 1e3)
        tt.sort()
        res["trimmed_prompt"] = {"p50_ms": tt[len(tt) // 2], "min_ms": tt[0], "prompt_slots": int(model._engine.T),
                                 "valid_prompt_tokens": int(obs.tokenized_prompt_mask.sum()),
                                 "note": "model.trim_prompt_padding_infer = True (the serve path's default); NOT the headline p50"}
    except Exception as e:  # noqa: BLE001
        res["trimmed_prompt"] = {"error": repr(e)[:200]}
    finally:
        model.trim_prompt_padding_infer = False
    mfma_floor = INFER_TFLOP / MFMA_BF16_PEAK_TFLOPS * 1e3
    hbm_floor = INFER_GB / (HBM_PEAK_TBS * 1e3) * 1e3
    res.update({
        "algorithmic_tflop": INFER_TFLOP, "algorithmic_gb": INFER_GB,
        "mfma_floor_ms": mfma_floor, "hbm_floor_ms": hbm_floor,
        "bound": "mfma" if mfma_floor >= hbm_floor else "hbm",
        "achieved_tflops": INFER_TFLOP / (p50 / 1e3), "achieved_gbs": INFER_GB / (p50 / 1e3),
        "frac": max(mfma_floor, hbm_floor) / p50,
        "target_ms": 15.0,
    })
    model.train()
    return res


def roofline_object(timer, timer_dual, timer_steps: int, B: int, ms_per_step: float) -> dict:
    """The `roofline` object of the JSON line from the GEMM timers (both schedules)."""
    gemm_ms, gemm_flops, n_launch = timer.summarize()
    # algorithmic flops of a launch = 2 M N K of that launch (no tile padding counted); summed over the launches
    # of the measured steps and divided by their summed HIP-event durations
    achieved = gemm_flops / 1e12 / (gemm_ms / 1e3)
    # PMC counters cannot be read from inside this process: the per-launch HBM-side bytes come from the committed
    # rocprofv3 --pmc passes over this same command (tools/collect_profiles.sh -> profiles/gemm_traffic.json)
    traffic = {}
    tpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "gemm_traffic.json")
    if os.path.exists(tpath):
        traffic = json.load(open(tpath))
    return {
        "bound": "mfma",
        "kernel": "gemm_bf16_kernel (NT/NN/TN variants; every Linear, attention matmul, dgrad and wgrad)",
        "achieved": achieved,
        "peak": MFMA_BF16_PEAK_TFLOPS,
        "unit": "TFLOP/s",
        "frac": achieved / MFMA_BF16_PEAK_TFLOPS,
        "traffic": traffic.get("bytes_per_launch"),
        "traffic_unit": "HBM-side bytes per GEMM launch (fetch + write), rocprofv3 PMC; not re-measured by this run",
        "traffic_measured_by_this_run": False,
        "traffic_source": traffic.get("source"),
        "traffic_commit": traffic.get("commit"),
        "traffic_date": traffic.get("date"),
        "launches_per_step": n_launch // timer_steps,
        "avg_launch_ms": gemm_ms / n_launch,
        "gemm_ms_per_step": gemm_ms / timer_steps,
        "algorithmic_tflop_per_step": TRAIN_TFLOP_PER_SAMPLE * B,
        "needed_tflop_per_step": TRAIN_TFLOP_NEEDED_PER_SAMPLE * B,
        "gemm_tflop_per_step": gemm_flops / timer_steps / 1e12,
        "timed": f"HIP events over {timer_steps} further identical steps right after the timed region, with the second "
                 "(action-expert) stream off so that every launch owns the chip while it is timed",
        "frac_timed_inside_timed_region": False,
        "frac_timed_steps": timer_steps,
        "frac_timed_expert_stream": False,
        "headline_schedule": (lambda ms, fl, n: {
            "frac": fl / 1e9 / ms / MFMA_BF16_PEAK_TFLOPS, "achieved": fl / 1e9 / ms, "gemm_ms_per_step": ms / timer_steps,
            "launches_per_step": n // timer_steps,
            "note": "the same HIP events over two further steps with the action expert's chain on its second stream, as in the timed "
                    "region: overlapping launches are each charged the time they share, so this is a lower bound per launch"})(*timer_dual.summarize())
        if timer_dual is not None else None,
        "step_frac_of_mfma_peak": TRAIN_TFLOP_NEEDED_PER_SAMPLE * B / (ms_per_step / 1e3) / MFMA_BF16_PEAK_TFLOPS,
        "step_frac_priced_on_tflop_per_sample": TRAIN_TFLOP_NEEDED_PER_SAMPLE,
        "families": timer.families(B, timer_steps),
        "targets": {"gemma_blocks_frac": 0.40, "vit_blocks_frac": 0.40},
        "peak_note": "peak = the guide's dense bf16 figure at 2.4 GHz; under these launches the socket sits at its 1400 W cap with the "
                     "shader clock at 1.8-2.1 GHz (profiles/r05_clock_power_under_gemm.txt, not re-measured by this run)",
    }


DUMP_SAMPLE = 4096  # elements per parameter in the --dump-outputs samples (all of a parameter that has fewer)


@torch.no_grad()
def dump_outputs(out_dir: str, trainer, loss) -> None:
    """What the last timed step computed, as float32 DIR/<name>.npy: `loss` (what train_step returns), `grad_norm` (the global
    pre-clip gradient norm), and of this rank's shard of the updated state the same fixed, seeded sample of every parameter
    (parameters in name order; positions drawn from a CPU generator seeded 0): `master` (the f32 weights after the update),
    `exp_avg` (AdamW's first moment) and `grad` (the step's gradient).  `grad` leaves out the parameters whose gradient producer
    accumulates into its slice (`_kai0_grad_accumulates`: the embedding table), because ShardedDataParallel.step zeroes those
    slices after the update; `master` and `exp_avg` cover them.  About 30 MB at one GPU."""
    import numpy as np

    eng = trainer.engine
    entries = sorted((n, b, o, p) for b in eng.buckets for n, p, o in zip(b.names, b.params, b.offsets))
    g = torch.Generator().manual_seed(0)
    picks = []
    for _, b, o, p in entries:
        n = p.numel()
        idx = torch.arange(n) if n <= DUMP_SAMPLE else torch.randint(n, (DUMP_SAMPLE,), generator=g)
        pos = idx + (o - b.lo)  # position in this rank's shard of the bucket
        pos = pos[(pos >= 0) & (pos < b.shard)]
        picks.append((b, pos.to(b.master.device), getattr(p, "_kai0_grad_accumulates", False)))
    arrays = {"loss": loss.reshape(1), "grad_norm": trainer.last_grad_norm.reshape(-1),
              "master": torch.cat([b.master[pos] for b, pos, _ in picks]),
              "exp_avg": torch.cat([b.exp_avg[pos] for b, pos, _ in picks]),
              "grad": torch.cat([b.grad_shard[pos].float() for b, pos, acc in picks if not acc])}
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.float().cpu().numpy())


def rank_census(device, world: int, per_rank_ms: list) -> dict:
    """Who took part, answered by the line itself: the world size RCCL reports, one all_gather of the ranks' device
    identities (uuid, else PCI bus id) and host names, and the per-rank step time of the timed region."""
    import socket

    import torch.distributed as dist

    props = torch.cuda.get_device_properties(device)
    ident = str(getattr(props, "uuid", "") or "") or f"pci:{getattr(props, 'pci_bus_id', '?')}:{getattr(props, 'pci_device_id', '?')}"
    mine = {"rank": int(os.environ.get("RANK", "0")), "local_rank": device.index, "device": ident, "name": props.name, "host": socket.gethostname(),
            "gcn_arch": getattr(props, "gcnArchName", "")}  # fmt: skip
    seen = [mine]
    if world > 1:
        seen = [None] * world
        dist.all_gather_object(seen, mine)
    return {
        "rccl_ranks_seen": dist.get_world_size() if dist.is_initialized() else 1,
        "backend": dist.get_backend() if dist.is_initialized() else None,
        "distinct_devices": len({(r["host"], r["device"]) for r in seen}),
        "devices": seen,
        "ms_per_step_per_rank": per_rank_ms,
        "ms_per_step_spread": max(per_rank_ms) - min(per_rank_ms),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-per-gpu", type=int, default=32)
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/*.npy")
    ap.add_argument("--full", action="store_true", help="also measure the extras (ranks, comm, roofline, trimmed prompt, inference, CPU baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-gemm-timing", action="store_true")
    ap.add_argument("--no-trim-extra", action="store_true")
    args = ap.parse_args()

    import torch.distributed as dist

    from kai0_amd.config import Pi0Config
    from kai0_amd.train import Trainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world > 1 or os.environ.get("KAI0_FORCE_COLLECTIVES") == "1":  # the latter: 1-rank RCCL dry run of the sharded path
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        # NCCL_DEBUG=VERSION (set on the bench boxes) makes RCCL print a banner through C stdio, which a pipe flushes at
        # process exit — i.e. AFTER the JSON line this script owes its caller as the last line of stdout.  Banner off;
        # anything else a user asked for (WARN, INFO, TRACE) stays, and every rank flushes C stdio before rank 0 prints.
        if os.environ.get("NCCL_DEBUG", "").upper() == "VERSION":
            del os.environ["NCCL_DEBUG"]
        dist.init_process_group(backend="nccl", init_method="env://", device_id=device)

    cfg = Pi0Config()
    B = args.batch_per_gpu
    model = build_model(cfg, device, seed=0)  # same weights on every rank
    model.train()
    # N > 1: the headline is north_star's partition — optimizer / gradients / PARAMETERS sharded ("fsdp": all-gather per unit ahead of
    # forward and backward, reduce-scatter from inside backward); zero2 (parameters resident: the natural mode with 288 GB per GPU) is
    # measured beside it (comm.zero2).  One GPU: nothing to shard, the engine's default.  KAI0_SHARD_MODE overrides.
    want_mode = os.environ.get("KAI0_SHARD_MODE") or ("fsdp" if world > 1 else "zero2")
    obs, actions = synthetic_batch(cfg, B, seed=1000 + rank, device=device)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def make_trainer(mode):
        return Trainer(model, world_size=world, rank=rank, peak_lr=2.5e-5, warmup_steps=1000, decay_steps=30000,
                       end_lr=2.5e-6, weight_decay=1e-10, clip_norm=1.0, mode=mode)  # fmt: skip

    # The first multi-GPU run of the fsdp partition happens on the driver's node, unattended: an error every rank raises alike while
    # the engine is built or during the first warm-up step (nothing has been timed yet) falls back to zero2 on a fresh model instead
    # of losing the line; the line says so (`headline_fallback`).  A hang is not an exception — nothing here can catch that.
    headline_fallback = None
    try:
        trainer = make_trainer(want_mode)
        if args.warmup > 0:
            trainer.train_step(obs, actions)
    except Exception as e:  # noqa: BLE001
        if world == 1 or want_mode == "zero2":
            raise
        headline_fallback = f"{want_mode} failed before the timed region ({type(e).__name__}: {str(e)[:300]}); headline measured in zero2"
        print(f"[bench] rank {rank}: {headline_fallback}", file=sys.stderr, flush=True)
        model.set_unit_hooks(None)
        del model
        torch.cuda.empty_cache()
        model = build_model(cfg, device, seed=0)
        model.train()
        trainer = make_trainer("zero2")
        if args.warmup > 0:
            trainer.train_step(obs, actions)
    for _ in range(max(0, args.warmup - 1)):
        trainer.train_step(obs, actions)
    # Timed region: exactly `steps` training steps between barriers, nothing else on the stream.
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = trainer.train_step(obs, actions)
    barrier()
    elapsed = time.perf_counter() - t0
    el = torch.tensor([elapsed], dtype=torch.float64, device=device)
    per_rank_ms = [elapsed / args.steps * 1e3]
    if world > 1:  # max over ranks, taken NOW: everything below is extra and must not be able to lose the headline
        every = [torch.zeros_like(el) for _ in range(world)]
        dist.all_gather(every, el)  # (the spread over ranks goes into the line: a straggler GPU shows up by itself)
        per_rank_ms = [float(t) / args.steps * 1e3 for t in every]
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, trainer, loss)
    ranks = None
    if args.full:
        try:
            ranks = rank_census(device, world, per_rank_ms)
        except Exception as e:  # noqa: BLE001 - diagnostics must never cost the headline
            ranks = {"error": f"{type(e).__name__}: {e}", "ms_per_step_per_rank": per_rank_ms}
    # Roofline of the dominant kernel: HIP events around every bf16 GEMM launch, over `timer_steps` further identical steps
    # right after the timed region (every rank steps, rank 0 measures).  Inside the timed region the 2 x 1417 event
    # records per step cost ~10 ms (1.7 %) and, at N > 1, would make rank 0 the straggler the max-over-ranks reports.
    timer = timer_dual = None
    timer_steps = 2
    if args.full and not args.no_gemm_timing:
        from kai0_amd import model as _model

        # every launch is timed ALONE: in the timed region above the action expert's chain (a few dozen small launches per
        # layer) runs on a second stream next to the PaliGemma tower's GEMMs (model.forward_joint), and two kernels that share
        # the chip would each be charged the other's time
        dual_was = _model.set_expert_stream(False)
        if rank == 0:
            timer = GemmTimer()
            timer.install()
        for _ in range(timer_steps):
            trainer.train_step(obs, actions)
        barrier()
        if timer is not None:
            timer.uninstall()
        _model.set_expert_stream(dual_was)
        # ... and the HEADLINE schedule's own figure: the same events with the expert stream back on.  Launches that share
        # the chip are each charged the time they overlap, so this fraction is a lower bound of what the launches achieve; it is the one
        # that belongs to the timed region's schedule.
        if dual_was:
            if rank == 0:
                timer_dual = GemmTimer()
                timer_dual.install()
            for _ in range(timer_steps):
                trainer.train_step(obs, actions)
            barrier()
            if timer_dual is not None:
                timer_dual.uninstall()
    # N > 1: what the collectives cost the compute stream.  Two further steps with the engine's wait bookkeeping on (events around
    # every place where the compute stream waits for a gather / reduce-scatter / the norm all-reduce, kai0_amd.sharded): per rank,
    # the ms per step the chip sat in those waits, i.e. the communication that overlap did NOT hide.  Outside the timed region for the
    # same reason as the GEMM timing.
    comm = None
    headline_mode = trainer.engine.mode
    if args.full and (world > 1 or os.environ.get("KAI0_FORCE_COLLECTIVES") == "1"):
        eng = trainer.engine
        eng.comm_profile = True
        eng.comm_report()
        barrier()
        tc0 = time.perf_counter()
        for _ in range(timer_steps):
            trainer.train_step(obs, actions)
        barrier()
        tc = (time.perf_counter() - tc0) / timer_steps * 1e3
        rep = eng.comm_report()
        eng.comm_profile = False
        mine = torch.tensor([rep["comm_exposed_ms"] / timer_steps, rep["all_gather_wait"] / timer_steps,
                             rep["reduce_scatter_wait"] / timer_steps, rep["norm_all_reduce"] / timer_steps, tc],
                            dtype=torch.float64, device=device)  # fmt: skip
        allr = [torch.zeros_like(mine) for _ in range(world)]
        if world > 1:
            dist.all_gather(allr, mine)
        else:
            allr = [mine]
        by = eng.comm_bytes_per_step()
        comm = {
            "mode": eng.mode, "rs_algo": eng.rs_algo, "buckets": len(eng.buckets), "bucket_mb": max(b.numel * b.flat_param.element_size() for b in eng.buckets) / 2**20,
            "comm_exposed_ms_per_rank": [float(t[0]) for t in allr],
            "all_gather_wait_ms_per_rank": [float(t[1]) for t in allr],
            "reduce_scatter_wait_ms_per_rank": [float(t[2]) for t in allr],
            "norm_all_reduce_ms_per_rank": [float(t[3]) for t in allr],
            "ms_per_step_while_measured": max(float(t[4]) for t in allr),
            "bytes_per_rank_per_step": by,
            "xgmi_gbs_if_fully_overlapped": by["total"] / 1e9 / (max(float(t[4]) for t in allr) / 1e3) if by["total"] else 0.0,
            "rccl_env": {k: os.environ[k] for k in ("NCCL_ALGO", "NCCL_PROTO", "NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS", "RCCL_MSCCL_ENABLE",
                                                    "RCCL_MSCCLPP_ENABLE", "KAI0_RS_ALGO") if k in os.environ},
            "measured": f"events on the compute stream around every collective wait, {timer_steps} steps after the timed region",
        }  # fmt: skip
    # N > 1: the OTHER partition measured next to the headline (headline fsdp -> zero2 beside it, and the other way round): a fresh
    # model + Trainer(mode=other), 2 warm-up + 4 timed steps, its own exposed-communication figures.  KAI0_BENCH_FSDP=0 skips it.
    other = None
    other_mode = "zero2" if headline_mode == "fsdp" else "fsdp"
    watchdog = None
    if comm is not None and os.environ.get("KAI0_BENCH_FSDP", "1") != "0":
        # The second partition is an extra.  If it hangs (a collective that never completes on some rank) the headline measured above
        # must still reach the caller: after KAI0_BENCH_WATCHDOG_S seconds (default 420) every rank leaves, rank 0 printing the line.
        import threading

        def give_up():
            if rank == 0:
                line = {
                    "metric": "train samples/sec pi0.5 full FT", "value": B * world * args.steps / elapsed, "unit": "samples/s", "n_gpus": world,
                    "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
                    "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
                    "data": "synthetic (3x224x224 RGB + 200 prompt tokens + 50x32 actions, resident in HBM; random-init weights)",
                    "config": {"workload": "pi0.5 full fine-tune bf16, batch 32 per MI355X, 3-cam 224x224 (BASELINE.json configs[1])",
                               "global_batch": B * world, "seq_len": 968 + 50, "parallelism": f"dp{world} ({headline_mode})", "final_loss": float(loss)},
                    "comm": comm,
                    "ranks": ranks,
                    "truncated": True,  # same schema as the full line minus the extras that had not been computed yet
                    "note": f"the extra measurement of the {other_mode} partition did not finish within the watchdog's limit and was abandoned; "
                            "the headline above was complete before it started",
                }  # fmt: skip
                if timer is not None:
                    try:
                        line["roofline"] = roofline_object(timer, timer_dual, timer_steps, B, elapsed / args.steps * 1e3)
                    except Exception as e:  # noqa: BLE001 - the headline must go out whatever the extras do
                        line["roofline_error"] = repr(e)[:200]
                print(json.dumps(line), flush=True)
            os._exit(0)

        def arm(seconds: float):
            t = threading.Timer(seconds, give_up)
            t.daemon = True
            t.start()
            return t

        #  the rebuild of the 3.6 B-parameter model gets its own allowance; the measurement's clock starts after it
        limit = float(os.environ.get("KAI0_BENCH_WATCHDOG_S", "420"))
        watchdog = arm(limit + 240.0)
        try:
            if os.environ.get("KAI0_BENCH_TEST_HANG") == "1":  # (tests the watchdog: tools/gpu_tests.sh does not set it)
                time.sleep(10**6)
            model.set_unit_hooks(None)
            del trainer, model
            torch.cuda.empty_cache()
            model = build_model(cfg, device, seed=0)
            model.train()
            trainer = Trainer(model, world_size=world, rank=rank, peak_lr=2.5e-5, warmup_steps=1000, decay_steps=30000,
                              end_lr=2.5e-6, weight_decay=1e-10, clip_norm=1.0, mode=other_mode)  # fmt: skip
            eng = trainer.engine
            watchdog.cancel()
            watchdog = arm(limit)  # model rebuilt: the measurement itself has `limit` seconds
            for _ in range(2):
                trainer.train_step(obs, actions)
            eng.comm_profile = True
            eng.comm_report()
            barrier()
            tf0 = time.perf_counter()
            for _ in range(4):
                loss2 = trainer.train_step(obs, actions)
            barrier()
            tf = (time.perf_counter() - tf0) / 4
            rep = eng.comm_report()
            eng.comm_profile = False
            mine = torch.tensor([tf, rep["comm_exposed_ms"] / 4], dtype=torch.float64, device=device)
            allr = [torch.zeros_like(mine) for _ in range(world)]
            if world > 1:
                dist.all_gather(allr, mine)
            else:
                allr = [mine]
            tmax = max(float(t[0]) for t in allr)
            other = {"mode": eng.mode, "samples_per_s": B * world / tmax, "ms_per_step": tmax * 1e3, "buckets": len(eng.buckets),
                     "prefetch": eng.prefetch, "comm_exposed_ms_per_rank": [float(t[1]) for t in allr],
                     "bytes_per_rank_per_step": eng.comm_bytes_per_step(), "final_loss": float(loss2),
                     "note": f"fresh Trainer(mode='{other_mode}') "
                             + ("(parameters sharded too, gathered two buckets ahead in forward and backward)" if other_mode == "fsdp"
                                else "(optimizer and gradients sharded, the bf16 model resident; all-gathers hidden behind the next forward)")
                             + "; 4 steps after 2 warm-up steps; NOT the headline value"}
        except Exception as e:  # noqa: BLE001 - the headline line must still be printed
            other = {"error": f"{type(e).__name__}: {e}"}
        watchdog.cancel()
        comm[other_mode] = other
    fsdp = other
    # Extra (not the headline value): the same step with the prompt cut to the longest valid prompt of the batch
    # (model.trim_prompt_padding: the 200 prompt slots carry 64-128 valid tokens here; padded slots are invisible keys and unread
    # rows, loss and gradients unchanged beyond summation order — tests/test_model_gpu.py).  The headline number above computes
    # all 200 slots, as the reference does.
    trimmed = None
    if args.full and world == 1 and not args.no_trim_extra:
        model.trim_prompt_padding = True
        for _ in range(2):
            trainer.train_step(obs, actions)
        barrier()
        t1 = time.perf_counter()
        for _ in range(4):
            trainer.train_step(obs, actions)
        barrier()
        tt = (time.perf_counter() - t1) / 4
        model.trim_prompt_padding = False
        keep = int(obs.tokenized_prompt_mask.to(torch.int32).sum(1).max())
        trimmed = {"samples_per_s": B / tt, "ms_per_step": tt * 1e3, "prompt_slots": (keep + 7) // 8 * 8,
                   "note": "model.trim_prompt_padding = True; 4 steps after 2 warm-up steps; NOT the headline value"}
    ms_per_step = elapsed / args.steps * 1e3
    value = B * world * args.steps / elapsed
    if world > 1:  # every rank empties its C stdio buffers (RCCL warnings) now, so nothing of theirs can follow rank 0's line
        import ctypes

        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        dist.barrier()

    if rank == 0:
        out = {
            "metric": "train samples/sec pi0.5 full FT",
            "value": value,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic (3x224x224 RGB + 200 prompt tokens + 50x32 actions, resident in HBM; random-init weights)",
            "config": {
                "workload": "pi0.5 full fine-tune bf16, batch 32 per MI355X, 3-cam 224x224 (BASELINE.json configs[1])",
                "global_batch": B * world,
                "seq_len": 968 + 50,
                "parallelism": f"dp{world}" + ("" if world == 1 else f" ({headline_mode}: sharded optimizer/grads"
                                                + ("/params" if headline_mode == "fsdp" else "") + ", RCCL reduce-scatter + all-gather"
                                                + (f"; {other_mode} measured beside it: comm.{other_mode}" if fsdp else "") + ")"),
                "params_stored": 3.617e9,
                "final_loss": float(loss),
            },
        }
        if timer is not None:
            out["roofline"] = roofline_object(timer, timer_dual, timer_steps, B, ms_per_step)
            if os.environ.get("KAI0_GEMM_BREAKDOWN"):
                os.makedirs("gpurun_out", exist_ok=True)
                json.dump(timer.breakdown(), open("gpurun_out/gemm_breakdown.json", "w"), indent=0)
        if comm is not None:
            out["comm"] = comm
        if headline_fallback is not None:
            out["headline_fallback"] = headline_fallback
        if ranks is not None:
            out["ranks"] = ranks
        if trimmed is not None:
            out["trimmed_prompt"] = trimmed
        if args.full and world == 1 and not args.no_latency:
            del trainer
            torch.cuda.empty_cache()
            out["inference"] = measure_latency(model, cfg, device)
            out["p50_action_chunk_ms"] = out["inference"]["p50_ms"]
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(B)
            cb_inf = out["cpu_baseline"].pop("inference", None)
            if cb_inf is not None and "inference" in out:
                out["inference"]["cpu_baseline"] = cb_inf
        try:  # whatever native libraries still hold in C stdio buffers goes out first: the JSON line must be the last one
            import ctypes

            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
