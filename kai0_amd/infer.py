"""Action-chunk inference engine: prefix pass into a static KV cache + Euler denoise loop, captured as one
hipGraph (pi0_pytorch.py:375-461; gemma_pytorch.py:102-125; modeling_gemma.py:282-329).

MI355X-first choices:
  * static, pre-allocated KV cache [layers][B, S_ld, HD]: the prefix pass writes rows [0, P), every denoise
    step overwrites rows [P, P+H) in place — no `torch.cat([cache, new])`, no DynamicCache;
  * projection GEMMs write straight into the padded q / K / V buffers (row-remap epilogue) and o_proj reads
    the attention output through the same remap: no concat/split copies;
  * o_proj / down_proj fuse the expert's gated residual (x + y*gate) into the GEMM epilogue;
  * the time schedule of the Euler loop is fixed (t = 1, 1+dt, ...), so the time-MLP conditioning and all
    37 adaRMS modulations for ALL steps are computed as M = steps*B row GEMMs (0.46 GB of f32 `dense` weights are
    read once instead of once per step) — and, being a function of the weights and the schedule only (no request input
    enters: sincos(t) -> time MLP -> `dense`), ONCE PER ENGINE, not per request: the engine is dropped whenever a weight
    changes (`_fingerprint`), so the table is constant for its lifetime, like the RoPE inverse frequencies.  Everything of this
    kind lives in ONE record per schedule (`_schedule`), built on the schedule's first run, outside graph capture;
  * the last prefix layer stops after its K/V projection — nothing reads its attention/MLP output;
  * the whole call (SigLIP -> prefix -> all denoise steps) is recorded once into a hipGraph
    (torch.cuda.CUDAGraph on ROCm is hipGraph) and replayed per request: no per-op Python or launch cost (`_Capture`);
  * one Euler driver, `_run`: schedule record, prefix pass, then either the production stack (`fast`: folded weights, in-block
    kernels, one-launch step seams — `_seams_pi05` / `_seams_pi0`) or the generic per-layer step `_denoise_step` over the plain GEMM;
  * pi0 (`pi05=False`): `state` is a request input (a static buffer of the graph), the suffix has Hs + 1 rows per
    sample (state token | action tokens, mask codes 0 / 1 / 2), the time half of `action_time_mlp_in` is hoisted per step like the
    modulation table, and the expert's plain RMSNorms run through the same folded stack as the constant modulation [w | 0 | 1].
    The generic step is the same function for both variants: what differs (rows per sample, the suffix embedding, the norm, the
    gate) is data;
  * real-time chunking: a request with a previous chunk runs the guided loop `_run_guided` — per Euler step one
    forward of the generic per-layer step that keeps what its backward needs, an explicit reverse sweep over the training backward's
    entry points (`_denoiser_vjp`) and two f32 seam kernels — captured into a hipGraph of its own; the unguided graph is not touched.
    Both variants: pi0's sweep carries all Hs + 1 suffix rows per sample, its plain norms as the constant modulation [w | 0 | 1], and ends
    behind the first layer in the suffix embedding's f32 Linears and SiLU.  `mask_prefix_delay` evaluates and linearises the denoiser at
    x_t with the delay rows overwritten by the previous chunk (kai0_rtc_overwrite) and updates the original x_t.
"""

from __future__ import annotations

import logging
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, ops
from . import lora as lora_ops
from .ops import BF16, F32, gemm, pick_split_k, round_up

logger = logging.getLogger("kai0_amd")
# split-K of the prefix pass's q|k|v, o_proj and down_proj GEMMs ("q,o,d"; 0 = ops.pick_split_k).  Swept on MI355X at B = 1
# (profiles/HISTORY.md): with the post-attention RMSNorm inside o_proj's reduction launch (kai0hip.h norm_kind) a split o_proj costs
# no extra launch: 1,2,6 -> prefix pass 5.56 ms against 5.68 for 1,1,6 (o = 3 and 4: 5.58 / 5.59); the automatic rule is 0.3 ms slower
_PREFIX_SPLITS = [int(x) for x in os.environ.get("KAI0_PREFIX_SPLITS", "1,2,6").split(",")]
# split-K of the SigLIP tower's two narrow-output Linears at B = 1 (M = 3 x 256 rows; (M, N, K) -> split), swept on MI355X (p50 of
# the tower, profiles/HISTORY.md): out_proj 54 tiles x 18 K-tiles unsplit + a LayerNorm launch -> three chunks with the norm inside the
# reduction launch; fc2 (K = 4304) four chunks (216 blocks, <= one per CU: the four-stage loop).  On the eight-wave 128 x 128 tile every
# other choice — (1 | 2, 4), (3, 2 | 3 | 6) — is +0.01 ... +0.27 ms against (3, 4), and prefix "1,1,6" / "1,2,8" / "1,2,4" +0.05 ... +0.1 ms
# against "1,2,6"
_B1_SPLITS = {(768, 1152, 1152): 3, (768, 1152, 4304): 4}


def NQ_ok(nq: int) -> bool:
    """contraction widths the in-block skinny kernel takes (K / 256 waves)"""
    return nq in (1024, 2048, 4096)


def euler_times(num_steps: int) -> list[float]:
    """The t values visited by `while time >= -dt/2` with f32 accumulation (pi0_pytorch.py:401-419)."""
    dt = np.float32(-1.0 / num_steps)
    t = np.float32(1.0)
    out = []
    while t >= -dt / 2:
        out.append(float(t))
        t = np.float32(t + dt)
    return out


class InferenceEngine:
    # test hooks (class attributes, read when an engine is built — not environment switches): the generic per-layer denoise path at
    # shapes the production stack would take, and the norms behind split-K Linears as launches of their own
    force_generic = False
    fuse_split_norm = True
    key_split = True  # B = 1 prefix attention as four key ranges of the one-pass kernel + merge (False: GEMM + softmax + GEMM)

    def __init__(self, model, batch: int, n_lang: int, n_cam: int):
        self.model = model
        pe = model.paligemma_with_expert
        self._pe_src = pe  # the parameters themselves: what `_fingerprint` and the content stamp watch
        # a LoRA model serves on merged weights W + s B A (kai0_amd.lora.merged_view): derived copies of this engine like the stacked
        # ones below, rebuilt with it when a base weight or an adapter changes
        self.pe = lora_ops.merged_view(pe) if lora_ops.has_adapters(pe) else pe
        self.B, self.T, self.ncam = batch, n_lang, n_cam
        self.n_img = pe.paligemma.model.vision_tower.vision_model.embeddings.num_patches
        self.P = n_cam * self.n_img + n_lang
        self.Hs = model.config.action_horizon
        self.A = model.config.action_dim
        self.pi05 = bool(model.pi05)
        self.n_state = 0 if self.pi05 else 1  # pi0: one continuous state token in front of the action tokens
        self.Ss = self.Hs + self.n_state  # suffix rows per sample
        self.S = self.P + self.Ss
        self.S_ld = round_up(self.S, 32)  # padded rows: 32-key groups of the decode attention never leave the buffers
        cfg = pe.vlm_cfg
        self.H, self.HD = cfg.num_heads, cfg.head_dim
        self.Dp, self.De = cfg.width, pe.exp_cfg.width
        self.L = cfg.depth
        dev = next(model.parameters()).device
        self.dev = dev
        B, S_ld, H, HD = self.B, self.S_ld, self.H, self.HD
        self.k_cache = [torch.zeros((B, S_ld, HD), dtype=BF16, device=dev) for _ in range(self.L)]
        self.v_all = torch.zeros((self.L, B, S_ld, HD), dtype=BF16, device=dev)
        self.v_cache = [self.v_all[l] for l in range(self.L)]
        self.q_buf = torch.zeros((B, S_ld, H * HD), dtype=BF16, device=dev)
        self.att_buf = torch.zeros((B, S_ld, H * HD), dtype=BF16, device=dev)
        self.use_graph = os.environ.get("KAI0_INFER_GRAPH", "1") != "0"
        # The production denoise stack (`fast`): weight-streaming in-block kernels with fused RoPE / GeGLU / gated-residual epilogues,
        # adaRMS folded into per-step weights, one-launch step seams, the two-launch decode attention — for the shapes it was built for
        # (few denoise rows, the pi0.5 widths, <= 1024 keys).  Anything else (the tiny test models, other widths) runs the generic
        # per-layer path `_denoise_step` over the plain GEMM.
        ecfg = pe.exp_cfg
        self.F = ecfg.mlp_dim
        # pi0 takes the same stack: a plain GemmaRMSNorm is the adaRMS arithmetic with the constant modulation [w | 0 | 1] (`_build_fast`)
        self.fast = (not self.force_generic and B * self.Ss <= 128 and ecfg.width == 1024 and NQ_ok(H * HD) and self.F in (1024, 2048, 4096) and HD == 256
                     and self.S <= 1024 and self.P % 8 == 0)  # fmt: skip
        self._weights_tag = self._fingerprint()
        if self.fast:
            self._build_fast()
        self._build_stacked()
        # the norm behind a split-K Linear of the SigLIP / prefix passes runs inside that Linear's reduction launch
        self.fuse_norm = bool(self.fuse_split_norm)
        self._schedules = {}  # tuple(times) -> the schedule's record (`_schedule`)
        self._cap = self._graph_steps = None  # the captured chunk (`_Capture`) and the step count baked into it
        # real-time chunking: the guided chunk's own capture, its key, and the previous chunk / prefix weights it reads
        self._g_cap = self._g_graph_key = None
        self._g_prev = self._g_w = self._g_delay = None
        self._content_init()

    # what tests, tools and the benchmark read of the captures
    _graph = property(lambda self: self._cap.graph if self._cap else None)
    _static_in = property(lambda self: self._cap.inputs if self._cap else None)
    _static_out = property(lambda self: self._cap.out if self._cap else None)
    _g_graph = property(lambda self: self._g_cap.graph if self._g_cap else None)

    @staticmethod
    def require_hip(device, what: str) -> None:
        """The guided sampler exists as HIP launches only — the taped step, the reverse sweep and the seams have no CPU form, and nothing
        falls back to eager torch: a model that is not on a HIP device is refused here, before any engine is built (the request's
        arguments have been validated by then: a bad one is a ValueError on any device)."""
        if torch.device(device).type != "cuda":
            raise NotImplementedError(f"{what} runs on the HIP engine only; the model's parameters are on `{device}`")

    def compatible(self, batch, n_lang, n_cam):
        return self.shape_matches(batch, n_lang, n_cam) and self.weights_unchanged()

    def shape_matches(self, batch, n_lang, n_cam) -> bool:
        return (batch, n_lang, n_cam) == (self.B, self.T, self.ncam)

    def weights_unchanged(self) -> bool:
        """The tensors the derived copies were cut from are the ones they were cut from (storage, autograd version, optimizer updates) and
        no completed chunk has stamped different contents.  ~0.13 ms of host time over ~470 tensors: `model.sample_actions` runs it AFTER
        it has queued the graph replay, so the check overlaps the chunk instead of standing in front of it; a mismatch discards
        that replay's result."""
        return self._weights_tag == self._fingerprint() and self._content_ok()

    # ---- content stamp of the source weights (the engine-invalidation contract, checked) ------------------------------------
    _CK_STRIDE = 128  # every 128th 64-byte unit: ~8 MB of the ~1 GB the derived copies were cut from, a few microseconds

    def _content_init(self):
        """The tensors of `_fingerprint` are also summed by content (kai0_sampled_checksum) at the end of every action chunk, inside
        the captured graph, and the sum lands in pinned host memory without a synchronisation.  `compatible()` compares the last
        landed sum with the one taken when the derived copies were built: an in-place edit that neither autograd's version counters
        nor the optimizer's update counter see (`p.data.mul_()`, a foreign kernel) drops the engine at the NEXT call at the latest
        — `stale()` tells a caller that has synchronised (Policy.infer) whether the chunk it just got was computed from edited
        weights, so the serve path never returns one.  Sampled: bulk edits (model arithmetic, a loaded checkpoint) are certain to
        be seen, a single edited element is not.  KAI0_INFER_CHECKSUM=0 disables the stamp."""
        self._ck_on = os.environ.get("KAI0_INFER_CHECKSUM", "1") != "0" and self.dev.type == "cuda"
        if not self._ck_on:
            return
        srcs = [p for p in self._fp_srcs if p.numel() * p.element_size() >= 64 and p.data_ptr() % 16 == 0 and p.is_contiguous()]
        self._ck_items = torch.tensor([[p.data_ptr(), p.numel() * p.element_size()] for p in srcs], dtype=torch.int64).to(self.dev)
        self._ck_n = len(srcs)
        self._ck_dev = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._ck_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self._content_stamp()
        torch.cuda.current_stream().synchronize()
        self._ck_ref = int(self._ck_host[0])

    def _content_stamp(self):
        if not self._ck_on:
            return
        self._ck_dev.zero_()
        _lib.call("kai0_sampled_checksum", self._ck_items.data_ptr(), self._ck_n, self._CK_STRIDE, self._ck_dev.data_ptr(), ops._stream())
        self._ck_host.copy_(self._ck_dev, non_blocking=True)

    def _content_ok(self) -> bool:
        """False once a completed chunk has stamped source weights that differ from the ones the derived copies were built from."""
        return not self._ck_on or int(self._ck_host[0]) == self._ck_ref

    def stale(self) -> bool:
        """After the caller has synchronised with the last chunk: was it computed while the source weights had been edited?"""
        return not self._content_ok()

    def _fingerprint(self):
        """Identity of the weights this engine (its stacked copies and its captured graph) was built from: storage and
        autograd version of every tensor a stacked copy was cut from, plus the count of optimizer updates made through the
        HIP kernels (they write through raw pointers, which autograd's version counters do not see).  An in-place edit that
        bypasses both (`p.data.copy_`, a foreign kernel) must be followed by `model.invalidate_inference_engine()`."""
        from . import optim

        cached = getattr(self, "_fp_srcs", None)
        if cached is not None:  # per request: one pass over the tensor list, no module-tree walk (~0.1 ms instead of ~0.5 ms of host time)
            return (optim.WEIGHT_UPDATES[0], *((p.data_ptr(), p._version) for p in cached))
        ex = self._pe_src.gemma_expert.model
        vt = self._pe_src.paligemma.model.vision_tower.vision_model
        lm = self._pe_src.paligemma.model.language_model
        srcs = [w for l in ex.layers for w in (l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight,
                                                l.mlp.gate_proj.weight, l.mlp.up_proj.weight, l.self_attn.o_proj.weight,
                                                l.mlp.down_proj.weight)]  # fmt: skip
        srcs += [w for l in lm.layers for w in (l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight)]
        for l in vt.encoder.layers:
            at = l.self_attn
            srcs += [at.q_proj.weight, at.k_proj.weight, at.v_proj.weight, at.q_proj.bias, at.k_proj.bias, at.v_proj.bias]
        m = self.model
        if self.pi05:
            srcs += [m for l in ex.layers for d in (l.input_layernorm.dense, l.post_attention_layernorm.dense) for m in (d.weight, d.bias)]
            srcs += [ex.norm.dense.weight, ex.norm.dense.bias]
            # the cached modulation table is cut from these too
            srcs += [m.time_mlp_in.weight, m.time_mlp_in.bias, m.time_mlp_out.weight, m.time_mlp_out.bias]
        else:  # pi0: the cached per-step time vectors are cut from action_time_mlp_in; the other heads are listed for the content stamp
            srcs += [w for l in ex.layers for w in (l.input_layernorm.weight, l.post_attention_layernorm.weight)] + [ex.norm.weight]
            srcs += [p for h in (m.state_proj, m.action_time_mlp_in, m.action_time_mlp_out) for p in (h.weight, h.bias)]
        if self.pe is not self._pe_src:  # merged weights: cut from every adapted Linear's base weight (the prefix tower's others too) and adapters
            srcs += [w for l in lm.layers for w in (l.self_attn.o_proj.weight, l.mlp.gate_proj.weight, l.mlp.up_proj.weight, l.mlp.down_proj.weight)]
            srcs += [p for n, p in self._pe_src.named_parameters() if ".lora_" in n]
        self._fp_srcs = srcs  # (the parameter OBJECTS are stable: load_state_dict / optimizer steps / .to() change data_ptr or _version)
        return (optim.WEIGHT_UPDATES[0], *((p.data_ptr(), p._version) for p in srcs))

    def _build_stacked(self):
        """q|k|v weights (and biases) stacked once per engine: one GEMM launch per attention block instead of three.
        (+0.2 GB SigLIP, +0.2 GB Gemma; the originals stay the checkpoint-visible parameters.)"""
        vt = self.pe.paligemma.model.vision_tower.vision_model
        self.sg_wqkv = [torch.cat([l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight], 0).contiguous()
                        for l in vt.encoder.layers]  # fmt: skip
        self.sg_bqkv = [torch.cat([l.self_attn.q_proj.bias, l.self_attn.k_proj.bias, l.self_attn.v_proj.bias], 0).contiguous()
                        for l in vt.encoder.layers]  # fmt: skip
        lm = self.pe.paligemma.model.language_model
        self.lm_wqkv = [torch.cat([l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight], 0).contiguous()
                        for l in lm.layers]  # fmt: skip
        # RoPE in the epilogue of the prefix pass's q|k|v GEMM (kai0hip.h act 7) where that GEMM runs on 128-column tiles (the
        # B = 1 pass: 18 launches of ~10 us fewer per chunk).  The rotation's partners (columns j, j + 128 of a head) must meet in one
        # tile, so the stacked copy of every layer but the last (which only projects K / V) is kept with its rows permuted instead.
        NQ = self.H * self.HD
        self.fuse_rope = self.HD == 256 and self.B * self.P <= 1024 and _PREFIX_SPLITS[0] in (0, 1)
        if self.fuse_rope:
            perm = ops.rope_permutation(NQ + 2 * self.HD, NQ + self.HD).to(self.dev)
            for l in range(self.L - 1):
                self.lm_wqkv[l] = self.lm_wqkv[l][perm].contiguous()

    def _gemm_norm(self, a, w, out, norm, plain: bool, **kw):
        """gemm(a, w, out [M, N], **kw), then the norm that reads `out`, norm = (kind, weight, bias | None, eps) or None: inside the
        split-K reduction launch (kai0hip.h norm_kind) when the contraction is split and the epilogue is `plain` (the caller's own
        term), otherwise as a launch of its own.  Returns out, or (out, norm(out))."""
        M, N = out.shape
        fused = None
        if norm is not None and self.fuse_norm and kw["split_k"] > 1 and N <= 2048 and N % 8 == 0 and plain:
            kind, nw, nb, neps = norm
            fused = (kind, torch.empty((M, N), dtype=BF16, device=self.dev), nw, nb, neps)
        gemm(a, w, out, norm=fused, **kw)
        if norm is None:
            return out
        if fused is not None:
            return out, fused[1]
        kind, nw, nb, neps = norm
        return out, (ops.rmsnorm(out, nw, neps) if kind == 1 else ops.layernorm(out, nw, nb, neps))

    def _lin(self, x, w, *, bias=None, residual=None, act=0, split=None, aux1=None, norm=None, out=None):
        """flat Linear for the prefix / SigLIP passes: launches matter more than occupancy here, so the contraction is
        only split when there are fewer than ~100 output tiles.  norm: the norm that reads this Linear's output (`_gemm_norm`)."""
        M, K = x.shape
        N = w.shape[0]
        if split is None:
            tiles = ((M + 127) // 128) * ((N + 127) // 128)
            split = _B1_SPLITS.get((M, N, K)) or (1 if tiles >= 100 else pick_split_k(M, N, K))
        if out is None:
            out = torch.empty((M, N), dtype=BF16, device=self.dev)
        return self._gemm_norm(x, w, out, norm, act == 0, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, residual=residual, ldr=N,
                               act=act, aux1=aux1, split_k=split)  # fmt: skip

    def _siglip(self, image, out=None):
        """SigLIP tower for inference (modeling_siglip.py:271-281,325-460,756-778): stacked q|k|v projection, attention
        straight off the stacked buffer, no probabilities written, GELU / bias / residual in the GEMM epilogues."""
        pe = self.pe
        vt = pe.paligemma.model.vision_tower.vision_model
        sc = pe.siglip_cfg
        n = image.shape[0]
        S = vt.embeddings.num_patches
        NH, HD = sc.num_heads, sc.hidden_size // sc.num_heads
        E = NH * HD
        emb = vt.embeddings
        x = ops.patch_embed(image.contiguous(), emb.patch_embedding.weight, emb.patch_embedding.bias,
                            emb.position_embedding.weight, sc.patch_size)  # fmt: skip
        scale = HD**-0.5
        layers = list(vt.encoder.layers)
        h = ops.layernorm(x, layers[0].layer_norm1.weight, layers[0].layer_norm1.bias, layers[0].layer_norm1.eps)
        for l, layer in enumerate(layers):
            qkv = self._lin(h, self.sg_wqkv[l], bias=self.sg_bqkv[l])
            a = torch.empty((n * S, E), dtype=BF16, device=self.dev)
            if S == 256 and HD == 72 and ops._SIGLIP_FWD_DEDICATED:  # the real tower: head-resident kernel, exact one-pass softmax
                ops.siglip_attn_fwd(qkv, qkv[:, E:], qkv[:, 2 * E:], a, n_img=n, S=S, NH=NH, HD=HD, ld_qkv=3 * E, ld_out=E)
            else:
                ops.attn_fwd(qkv, qkv[:, E:], qkv[:, 2 * E:], a, None, rows=S, Sk=S, HD=HD, H=1, batch=n * NH, batch_inner=NH,
                             ldq=3 * E, ldk=3 * E, ldv=3 * E, ldo=E, sQ=(S * 3 * E, HD), sK=(S * 3 * E, HD), sV=(S * 3 * E, HD),
                             sO=(S * E, HD), scale=scale)  # fmt: skip
            # each norm is handed to the Linear that produces its input (out_proj -> layer_norm2, fc2 -> the next layer's layer_norm1 /
            # the post-layernorm): split-K Linears run it inside their reduction launch
            ln2 = layer.layer_norm2
            x, h = self._lin(a, layer.self_attn.out_proj.weight, bias=layer.self_attn.out_proj.bias, residual=x,
                             norm=(2, ln2.weight, ln2.bias, ln2.eps))  # fmt: skip
            f = self._lin(h, layer.mlp.fc1.weight, bias=layer.mlp.fc1.bias, act=1)
            nxt = layers[l + 1].layer_norm1 if l + 1 < len(layers) else vt.post_layernorm
            x, h = self._lin(f, layer.mlp.fc2.weight, bias=layer.mlp.fc2.bias, residual=x, norm=(2, nxt.weight, nxt.bias, nxt.eps))
        x = h  # = post_layernorm(x)
        proj = pe.paligemma.model.multi_modal_projector.linear
        return self._lin(x, proj.weight, bias=proj.bias, out=out).view(n, S, -1)  # (`out`: the prefix buffer's image rows, B = 1)

    def _embed_prefix(self, images, img_masks, lang_tokens, lang_masks):
        """PI0Pytorch.embed_prefix (pi0_pytorch.py:186-235) over the inference SigLIP tower -> the flat prefix [B * P, D].  No
        assembly copies — the prompt embedding is gathered straight into its rows of the prefix buffer (kai0_embed_gather's row offset /
        strides) and, at B = 1 (where camera-major == sequence order), the projector GEMM writes the image rows there too; the pad / att
        masks are not materialised (kai0_prefix_codes, `_prefix_pass`)."""
        pe = self.pe
        B, ncam = lang_tokens.shape[0], len(images)
        n_img, D, T = self.n_img, self.Dp, lang_tokens.shape[1]
        P = ncam * n_img + T
        embs = torch.empty((B * P, D), dtype=BF16, device=self.dev)
        direct = B == 1
        feats = self._siglip(torch.cat(images, dim=0), out=embs[: ncam * n_img] if direct else None)
        if feats.shape[2] != D:
            raise ValueError(f"prefix assembly: projector width {feats.shape[2]} != PaliGemma width {D}")
        tok = lang_tokens.to(torch.int64).contiguous() if lang_tokens.dtype != torch.int64 else lang_tokens.contiguous()
        table = pe.paligemma.model.language_model.embed_tokens.weight
        ops.embed_gather(table, tok, embs, ops.sqrt_scale(D), P * D, ncam * n_img, D)
        if not direct:
            for c, cam in enumerate(feats.reshape(ncam, B, n_img, D)):
                ops.copy_rows(cam, embs.view(B, P, D)[:, c * n_img : (c + 1) * n_img])
        return embs.view(B, P, D)

    def _build_fast(self):
        ex = self.pe.gemma_expert.model
        B, HD, dev = self.B, self.HD, self.dev
        # stacked copies (0.5 GB): q|k|v and gate|up become one weight stream and one launch each; the in-block kernels stream the
        # weights as fragment-major 1-KiB blocks (ops.pack_skinny_weight): every wave-instruction of the stream is one contiguous KiB
        # instead of sixteen 64-B pieces of sixteen rows.  The row-major stacked copies are what the folded per-step weights are cut from.
        self.w_qkv_raw = [torch.cat([l.self_attn.q_proj.weight, l.self_attn.k_proj.weight, l.self_attn.v_proj.weight], 0).contiguous()
                          for l in ex.layers]  # fmt: skip
        self.w_gu_raw = [torch.cat([l.mlp.gate_proj.weight, l.mlp.up_proj.weight], 0).contiguous() for l in ex.layers]
        self.w_o = [ops.pack_skinny_weight(l.self_attn.o_proj.weight) for l in ex.layers]
        self.w_d = [ops.pack_skinny_weight(l.mlp.down_proj.weight) for l in ex.layers]
        # decode attention: needs the value cache transposed ([HD][keys])
        self.vt_all = torch.zeros((self.L, B, HD, self.S_ld), dtype=BF16, device=dev)
        if not self.pi05:
            # pi0: the expert's norms are plain GemmaRMSNorms, x_hat (1 + w) (modeling_gemma.py:77-81) — the adaRMS arithmetic with the
            # constant modulation row [scale = w | shift = 0 | gate = 1]: (x_hat (1 + w)) + 0.0 and x + y * 1.0 round nowhere (compare :80
            # with :102, and `_gated_residual` :209-227 with gate None).  Folded: W' = bf16(W (1 + w)), cvec = 0 — ONE packed set per
            # layer for all steps (0.4 GB against pi0.5's per-(step, layer) 4 GB), no gates (the kernels' plain residual epilogue).
            per_layer = []
            for l, layer in enumerate(ex.layers):
                ent = []
                for w, nw in ((self.w_qkv_raw[l], layer.input_layernorm.weight), (self.w_gu_raw[l], layer.post_attention_layernorm.weight)):
                    wp = (w.float() * (1.0 + nw.float())[None, :]).to(BF16)
                    ent.append((ops.pack_skinny_weight(wp), torch.zeros(w.shape[0], dtype=F32, device=dev)))
                per_layer.append(ent)
            self._plain_fold = per_layer
            De = self.De
            self._mod_final = torch.cat([ex.norm.weight.float(), torch.zeros(De, dtype=F32, device=dev),
                                         torch.ones(De, dtype=F32, device=dev)]).reshape(1, 3 * De).contiguous()
            return
        # all 37 adaRMS `dense` layers stacked: the modulations of every layer and step come out of ONE f32 GEMM
        dens = [m for l in ex.layers for m in (l.input_layernorm.dense, l.post_attention_layernorm.dense)] + [ex.norm.dense]
        self.w_mod = torch.cat([m.weight for m in dens], 0).contiguous()
        self.b_mod = torch.cat([m.bias for m in dens], 0).contiguous()

    # ---------------------------------------------------------------------------------------------- attention
    def _attend(self, l: int, q0: int, Sq: int, Sk: int, qcode, kcode, want_probs: bool = False):
        """masked MQA over the static buffers for query rows [q0, q0+Sq) against key rows [0, Sk).  want_probs (the guided step's forward,
        whose reverse sweep reads them): the logits / softmax / P V form at every batch, returns the probabilities bf16 [B, Sq H, S_ld]."""
        B, S_ld, H, HD = self.B, self.S_ld, self.H, self.HD
        M = Sq * H
        if not want_probs and ((M + 127) // 128) * B >= 192:  # enough 128-row blocks to fill the chip: one fused kernel
            ops.attn_fwd(self.q_buf, self.k_cache[l], self.v_cache[l], self.att_buf, None, rows=M, Sk=Sk, HD=HD, H=H, q0=q0,
                         batch=B, ldq=HD, ldk=HD, ldv=HD, ldo=HD, sQ=(S_ld * H * HD, 0), sK=(S_ld * HD, 0),
                         sV=(S_ld * HD, 0), sO=(S_ld * H * HD, 0), qcode=qcode, kcode=kcode, scale=HD**-0.5,
                         q_off=q0 * H * HD, o_off=q0 * H * HD)
            return
        if not want_probs and B == 1 and self.key_split and Sq > 128 and HD == 256 and Sk % 4 == 0 and Sk >= 512 and q0 == 0:
            # the B = 1 prefix pass: the one-pass kernel over four key ranges (244 blocks instead of 61) + the lse-weighted
            # merge — two launches and no logits / probabilities in memory instead of logits GEMM, softmax, split-K P V (+ reduce)
            ops.attn_fwd_keysplit(self.q_buf, self.k_cache[l], self.v_cache[l], self.att_buf, rows=M, Sk=Sk, HD=HD, H=H, q0=q0, ldk=HD, ldv=HD,
                                  qcode=qcode[0], kcode=kcode[0], scale=HD**-0.5, q_off=q0 * H * HD, o_off=q0 * H * HD, parts=4)
            return
        # latency-bound small batch: the key dimension has to be spread over the chip -> logits GEMM (N = keys),
        # masked softmax, split-K P V GEMM
        scores = torch.empty((B, M, S_ld), dtype=BF16, device=self.dev)
        gemm(self.q_buf, self.k_cache[l], scores, M=M, N=S_ld, K=HD, lda=HD, ldb=HD, ldc=S_ld, batch=B,
             sA=(S_ld * H * HD, 0), sB=(S_ld * HD, 0), sC=(M * S_ld, 0), scale=HD**-0.5, a_off_elems=q0 * H * HD)  # fmt: skip
        _lib.call("kai0_softmax_mask_fwd", scores.data_ptr(), scores.data_ptr(), qcode.data_ptr(), kcode.data_ptr(), B,
                  Sq, H, Sk, S_ld, M * S_ld, q0, qcode.stride(0), kcode.stride(0), ops._stream())  # fmt: skip
        gemm(scores, self.v_cache[l], self.att_buf, M=M, N=HD, K=S_ld, a_kc=True, b_kc=False, lda=S_ld, ldb=HD, ldc=HD,
             batch=B, sA=(M * S_ld, 0), sB=(S_ld * HD, 0), sC=(S_ld * H * HD, 0), c_off_elems=q0 * H * HD,
             split_k=pick_split_k(M, HD, S_ld, B))  # fmt: skip
        return scores

    def _proj_into(self, x, lin, dst, rows_pb: int, row0: int, width: int):
        """dst[b, row0 + r, :width] = (x @ W^T)[b*rows_pb + r]  — GEMM epilogue row remap, no copy."""
        M, K = x.shape
        gemm(x, lin.weight, dst, M=M, N=width, K=K, lda=K, ldb=K, ldc=width, c_map=(rows_pb, self.S_ld, row0),
             split_k=pick_split_k(M, width, K))

    def _oproj(self, lin, rows_pb: int, row0: int, residual, gate=None, norm=None):
        """y = att_buf[b, row0 + r] @ Wo^T (+gate) + residual, reading the padded buffer through the A row remap.
        norm: the norm that reads y (`_gemm_norm`)."""
        B, H, HD = self.B, self.H, self.HD
        M = B * rows_pb
        N = lin.weight.shape[0]
        out = torch.empty((M, N), dtype=BF16, device=self.dev)
        split = (_PREFIX_SPLITS[1] if M > 128 else 0) or pick_split_k(M, N, H * HD)
        return self._gemm_norm(self.att_buf, lin.weight, out, norm, gate is None, M=M, N=N, K=H * HD, lda=H * HD, ldb=H * HD, ldc=N,
                               a_map=(rows_pb, self.S_ld, row0), residual=residual, ldr=N, gate=gate, gate_rpb=rows_pb, gate_ld=N,
                               split_k=split)  # fmt: skip

    # ------------------------------------------------------------------------------------------------ passes
    def _prefix_pass(self, images, img_masks, lang_tokens, lang_masks):
        """Prefix rows through the PaliGemma tower into the static K / V caches; leaves the request's mask codes, position ids and the
        RoPE inverse frequencies on the engine for the denoise steps."""
        B, P, Hs = self.B, self.P, self.Hs
        prefix = self._embed_prefix(images, img_masks, lang_tokens, lang_masks)
        # mask codes and position ids of the whole request (prefix + action tokens) in one launch: what build_mask_codes makes of
        # embed_prefix's / embed_suffix's pad and att masks, bit for bit (tests/test_kernels_gpu.py::test_prefix_codes_...)
        qcode, kcode, pos = ops.prefix_codes([m.to(torch.bool) for m in img_masks], lang_masks.to(torch.bool), self.n_img, Hs,
                                             n_state=self.n_state)
        self.qcode, self.kcode, self.pos = qcode, kcode, pos
        self.pos_prefix = pos[:, :P].contiguous()
        self.pos_suffix = pos[:, P:].contiguous()
        lm = self.pe.paligemma.model.language_model
        self._inv_freq = inv_freq = lm.rope_inv_freq()
        H, HD, S_ld = self.H, self.HD, self.S_ld
        xp = prefix.reshape(B * P, self.Dp)
        NQ = H * HD
        M = B * P
        lm_layers = list(lm.layers)
        hp = ops.rmsnorm(xp, lm_layers[0].input_layernorm.weight, lm_layers[0].input_layernorm.eps)
        if self.fuse_rope:  # the rotation's tables for the prefix rows of this request, once per chunk (bf16: the values are bf16-rounded)
            rope_cos, rope_sin = ops.rope_table(self.pos_prefix.reshape(-1), inv_freq, bf16=True)
        for l, layer in enumerate(lm_layers):
            at = layer.self_attn
            if l == self.L - 1:
                # nothing consumes the last prefix layer's attention / MLP output: only its K and V rows are needed
                gemm(hp, self.lm_wqkv[l][NQ:], self.k_cache[l], M=M, N=2 * HD, K=self.Dp, lda=self.Dp, ldb=self.Dp, ldc=HD,
                     c_map=(P, S_ld, 0), segs=[(self.k_cache[l], HD, 0), (self.v_cache[l], HD, HD)],
                     split_k=pick_split_k(M, 2 * HD, self.Dp))  # fmt: skip
                ops.rope_(self.k_cache[l][:, :P], self.pos_prefix, inv_freq, HD)
                break
            # stacked q|k|v projection written straight into the padded q buffer and the K / V caches
            segs = [(self.q_buf, NQ, 0), (self.k_cache[l], HD, NQ), (self.v_cache[l], HD, NQ + HD)]
            if self.fuse_rope:  # ... rotated on the way out (rows of the stacked weight permuted, _build_stacked)
                gemm(hp, self.lm_wqkv[l], self.q_buf, M=M, N=NQ + 2 * HD, K=self.Dp, lda=self.Dp, ldb=self.Dp, ldc=NQ,
                     c_map=(P, S_ld, 0), segs=segs, act=7, rope=(rope_cos, rope_sin, HD // 2, NQ + HD))
            else:
                gemm(hp, self.lm_wqkv[l], self.q_buf, M=M, N=NQ + 2 * HD, K=self.Dp, lda=self.Dp, ldb=self.Dp, ldc=NQ,
                     c_map=(P, S_ld, 0), segs=segs, split_k=_PREFIX_SPLITS[0] or 1)
                ops.rope2_(self.q_buf[:, :P], self.k_cache[l][:, :P], self.pos_prefix, inv_freq, HD)  # q and k: one launch
            self._attend(l, 0, P, P, qcode, kcode)
            pan = layer.post_attention_layernorm
            xp, hp = self._oproj(at.o_proj, P, 0, residual=xp, norm=(1, pan.weight, None, pan.eps))
            wg, wu = layer.mlp.gate_proj.weight, layer.mlp.up_proj.weight
            if ops._GEGLU_PAIR and wg.shape[0] % 32 == 0:
                # gate | up as one GEMM over both weights, GeGLU in registers: only h is written
                hmid = torch.empty((M, wg.shape[0]), dtype=BF16, device=self.dev)
                gemm(hp, wg, hmid, M=M, N=wg.shape[0], K=self.Dp, lda=self.Dp, ldb=self.Dp, ldc=wg.shape[0], act=6, B2=wu)
            else:
                g = self._lin(hp, wg)
                hmid = self._lin(hp, wu, act=2, aux1=g)  # GeGLU in the epilogue
            nxt = lm_layers[l + 1].input_layernorm  # (the loop leaves at the last layer: there is always a next one here)
            xp, hp = self._lin(hmid, layer.mlp.down_proj.weight, residual=xp, norm=(1, nxt.weight, None, nxt.eps),
                               split=_PREFIX_SPLITS[2] or pick_split_k(M, self.Dp, hmid.shape[1]))

    def _schedule(self, times: list[float]):
        """The record of one Euler schedule: everything that is a function of the weights and the time values only — the engine is
        dropped when a weight changes, so it is kept for the engine's lifetime.  Built on the schedule's first (warm-up) run, OUTSIDE
        graph capture (the time values reach the device by a host-to-device copy).  Fields: pi0.5 — `times_dev` f32 [steps B], the
        modulation table `mods` / `mf` (`_modulations`); production stack: its row stride `mod_ld`, the bf16 `gates`, the `folded`
        per-step weights, and `guided` (contiguous `mods` / `mf` for the guided loop, made when first asked for); pi0 — `tvec`,
        `w_act` (`_time_vectors`)."""
        sch = self._schedules.get(tuple(times))
        if sch is None:
            sch = self._schedules[tuple(times)] = SimpleNamespace(times_dev=None, mods=None, mf=None, mod_ld=None, gates=None, folded=None,
                                                                  guided=None, tvec=None, w_act=None)  # fmt: skip
            if self.pi05:
                sch.times_dev = torch.tensor(times, dtype=F32).repeat_interleave(self.B).to(self.dev)
                sch.mods, sch.mf, sch.mod_ld, sch.gates = self._modulations(sch.times_dev)
                if self.fast:
                    sch.folded = self._fold_modulations(sch.mods, len(times))
            else:
                sch.tvec, sch.w_act = self._time_vectors(times)
        return sch

    def _guided_schedule(self, times: list[float]):
        """`mods` / `mf` of a schedule for the guided loop, which runs the generic per-layer step on every engine.  pi0.5: contiguous
        [steps B, 3 De] modulation rows per norm (the production stack keeps them as column slices of one table).  pi0: the schedule's
        `tvec` / `w_act`, and per norm the constant modulation rows [scale = w | shift = 0 | gate = 1] as f32 [B, 3 De] — the plain
        RMSNorm as adaRMS arithmetic (`_build_fast`), which hands the taped forward its rstd and the sweep its norm backward."""
        sch = self._schedule(times)
        if self.pi05 and not self.fast:
            return sch
        if sch.guided is None:
            if self.pi05:
                sch.guided = SimpleNamespace(mods=[(a.contiguous(), b.contiguous()) for a, b in sch.mods], mf=sch.mf.contiguous())
            else:
                ex, De, dev = self.pe.gemma_expert.model, self.De, self.dev

                def const_rows(ln):
                    row = torch.cat([ln.weight.float(), torch.zeros(De, dtype=F32, device=dev), torch.ones(De, dtype=F32, device=dev)])
                    return row.reshape(1, 3 * De).repeat(self.B, 1).contiguous()

                sch.guided = SimpleNamespace(mods=[(const_rows(l.input_layernorm), const_rows(l.post_attention_layernorm)) for l in ex.layers],
                                             mf=const_rows(ex.norm), tvec=sch.tvec, w_act=sch.w_act)  # fmt: skip
        return sch.guided

    def _modulations(self, tt):
        """time embedding -> time MLP -> adaRMS `dense` for every layer and step at once (rows = step*B + b; tt: the steps' time
        values, each B times).  -> (mods, mf, mod_ld, gates): per-layer (input norm, post-attention norm) modulations and the final
        norm's.  Production stack: one f32 GEMM over the 37 stacked `dense` weights, mods / mf its column views of row stride mod_ld,
        gates its bf16 cast (`_gate`); generic path: one GEMM per norm, no mod_ld / gates."""
        model, De = self.model, self.De
        te = ops.time_sincos(tt, De)
        x = ops.silu_f32(ops.linear_f32(te, model.time_mlp_in.weight, model.time_mlp_in.bias))
        cond = ops.silu_f32(ops.linear_f32(x, model.time_mlp_out.weight, model.time_mlp_out.bias))
        if not self.fast:
            ex = self.pe.gemma_expert.model
            mods = [(ops.linear_f32(cond, l.input_layernorm.dense.weight, l.input_layernorm.dense.bias),
                     ops.linear_f32(cond, l.post_attention_layernorm.dense.weight, l.post_attention_layernorm.dense.bias))
                    for l in ex.layers]  # fmt: skip
            return mods, ops.linear_f32(cond, ex.norm.dense.weight, ex.norm.dense.bias), None, None
        allm = ops.linear_f32(cond, self.w_mod, self.b_mod)  # [n*B, 37 * 3 De]
        gates = ops.cast(allm, BF16)  # gate = bf16(third chunk): taken as views, row stride mod_ld
        W3 = 3 * De
        mods = [(allm[:, (2 * l) * W3 : (2 * l + 1) * W3], allm[:, (2 * l + 1) * W3 : (2 * l + 2) * W3]) for l in range(self.L)]
        return mods, allm[:, 2 * self.L * W3 :], allm.shape[1], gates

    def _fold_modulations(self, mods, n_steps: int):
        """The adaRMS norms in front of the expert's q|k|v and gate|up projections, folded into the weights (kai0hip.h rowsq_in): the
        modulation of a step is a function of the step's time value and the weights only — the same for every request and every
        sample of the batch — so with W' = bf16(W (1 + scale)) and c = W shift the projection of the normalised activations is
        rstd * (x W'^T) + c on the RAW residual stream.  One packed W' and one c per (step, layer, projection): 10 x 18 x (5.2 + 16.8 MB)
        = 4 GB of the 288 GB, built once per engine; the kernels then carry no row-statistics pass and no per-element normalisation."""
        De = self.De
        out = []
        for step in range(n_steps):
            r = step * self.B  # (every row of a step holds the same modulation: the time value is shared by the batch)
            per_layer = []
            for l in range(self.L):
                ent = []
                for w, m in ((self.w_qkv_raw[l], mods[l][0]), (self.w_gu_raw[l], mods[l][1])):
                    scale, shift = m[r, :De], m[r, De : 2 * De]
                    wf = w.float()
                    wp = (wf * (1.0 + scale)[None, :]).to(BF16)
                    # c = W shift through the library's own exact-f32 GEMM (kai0_gemm_f32), not torch's matmul (rocBLAS gemv)
                    cvec = ops.linear_f32(shift.reshape(1, De).contiguous(), wf).reshape(-1)
                    ent.append((ops.pack_skinny_weight(wp), cvec.contiguous()))
                per_layer.append(ent)
            out.append(per_layer)
        return out

    def _gate(self, sch, idx: int, step: int):
        """bf16 gate vectors of stacked modulation `idx` (2 l: input norm, 2 l + 1: post-attention norm) for the rows of `step`."""
        B, De = self.B, self.De
        c0 = idx * 3 * De + 2 * De
        return sch.gates[step * B : (step + 1) * B, c0 : c0 + De]

    def _expert_layer_folded(self, l: int, xs, sq, parts: int, step: int, sch, rope):
        """Expert layer `l` of one denoise step, 6 launches and no partial products: [q|k|v + RoPE], logits, softmax + P V, [o_proj +
        gated residual], [gate|up + GeGLU], [down_proj + gated residual], with the adaRMS norms folded into the weights: the projections
        read the raw residual stream, the producers (denoise glue, o_proj, down_proj) hand the rows' partial sums of squares along (`sq`:
        [parts, M] f32); the gates are precomputed for all steps (`_gate`).  sch: the schedule's record; rope: the request's suffix
        (cos, sin) tables.  Returns (xs, sq, parts) for the next layer."""
        B, P, De, H, HD, S_ld, F = self.B, self.P, self.De, self.H, self.HD, self.S_ld, self.F
        Hs = self.Ss  # suffix rows per sample (pi0: the state token + the action tokens)
        M, dev = B * Hs, self.dev
        cos, sin = rope
        layer = self.pe.gemma_expert.model.layers[l]
        NQ = H * HD
        ada = self.pi05  # pi0: plain residuals (no gate operand), one folded weight set for all steps (`_plain_fold`)
        ld = sch.mod_ld if ada else 0
        (wq, cq), (wg, cg) = sch.folded[step][l] if ada else self._plain_fold[l]
        ops.skinny_gemm(xs, wq, M=M, N=NQ + 2 * HD, K=De, lda=De, ldw=De, mode=1, pair_stride=HD // 2, split_k=-1,
                        segs=[(self.q_buf, NQ, 0, NQ, 1), (self.k_cache[l], HD, NQ, NQ + HD, 1),
                              (self.vt_all[l], S_ld, NQ + HD, NQ + 2 * HD, 2)],
                        c_map=(Hs, S_ld, P), rope_cos=cos, rope_sin=sin, rope_half=HD // 2, eps=layer.input_layernorm.eps,
                        w_packed=True, rowsq_in=sq, rowsq_parts=parts, cvec=cq)  # fmt: skip
        ops.attn_decode(self.q_buf, self.k_cache[l], self.vt_all[l], self.att_buf, self.qcode, self.kcode, batch=B,
                        rows=Hs * H, H=H, HD=HD, Sk=P + Hs, q0=P, q_bs=S_ld * NQ, k_bs=S_ld * HD, k_ld=HD, k_rows=S_ld,
                        vt_bs=HD * S_ld, vt_ld=S_ld, scale=HD**-0.5)  # fmt: skip
        x1 = torch.empty((M, De), dtype=BF16, device=dev)
        sq1 = torch.empty((De // 16, M), dtype=F32, device=dev)
        ops.skinny_gemm(self.att_buf, self.w_o[l], M=M, N=De, K=NQ, lda=NQ, ldw=NQ, split_k=-1,
                        a_map=(Hs, S_ld, P), segs=[(x1, De, 0, De, 0)], gate=self._gate(sch, 2 * l, step) if ada else None, gate_rpb=Hs,
                        gate_ld=ld, residual=xs, ldr=De, w_packed=True, rowsq_out=sq1)  # fmt: skip
        h = torch.empty((M, F), dtype=BF16, device=dev)
        ops.skinny_gemm(x1, wg, M=M, N=2 * F, K=De, lda=De, ldw=De, mode=2, pair_stride=F, split_k=-1,
                        segs=[(h, F, 0, F, 0)], eps=layer.post_attention_layernorm.eps, w_packed=True,
                        rowsq_in=sq1, rowsq_parts=De // 16, cvec=cg)  # fmt: skip
        xs = torch.empty((M, De), dtype=BF16, device=dev)
        sq = torch.empty((De // 16, M), dtype=F32, device=dev)
        ops.skinny_gemm(h, self.w_d[l], M=M, N=De, K=F, lda=F, ldw=F, split_k=-1, segs=[(xs, De, 0, De, 0)],
                        gate=self._gate(sch, 2 * l + 1, step) if ada else None, gate_rpb=Hs, gate_ld=ld, residual=x1, ldr=De, w_packed=True,
                        rowsq_out=sq)  # fmt: skip
        return xs, sq, De // 16

    def _expert_stack_folded(self, xs, sq, step: int, sch, rope):
        """All expert layers of one denoise step (the step seam, kai0_denoise_glue, applies the final norm)."""
        parts = sq.shape[0]  # the step's first rows come from the glue kernel (one partial per row) / pi0's suffix embedding (De / 16)
        for l in range(self.L):
            xs, sq, parts = self._expert_layer_folded(l, xs, sq, parts, step, sch, rope)
        return xs

    def _time_vectors(self, times: list[float]):
        """pi0: the time half of `action_time_mlp_in` for every step of the schedule, tvec[step] = W_in[:, De:2De] time_emb(t_step) + b_in
        (f32 [steps, De]) — a function of the weights and the schedule only, like pi0.5's modulation table: once per engine, through
        the library's exact-f32 GEMM.  The action half W_in[:, :De] is kept as a contiguous copy next to it."""
        model, De = self.model, self.De
        tt = torch.tensor(times, dtype=F32).to(self.dev)
        te = ops.time_sincos(tt, De)
        w = model.action_time_mlp_in.weight
        tvec = ops.linear_f32(te, w[:, De:].contiguous(), model.action_time_mlp_in.bias)
        return tvec, w[:, :De].contiguous()

    def _pi0_suffix_embed(self, x_t, step: int, sch, xs):
        """pi0 embed_suffix of one denoise step (pi0_pytorch.py:263-285) into the action rows 1 .. Hs of every sample's Hs + 1 suffix rows
        `xs` (row 0, the state token, is constant for a request: `_pi0_state_rows` writes it once): action_in_proj, the action half of
        action_time_mlp_in + the step's hoisted time vector, SiLU, action_time_mlp_out — f32, one bf16 rounding at the store.
        Returns the SiLU's input f32 [B Hs, De] (what a guided step's reverse sweep keeps)."""
        model, B, Hs, De = self.model, self.B, self.Hs, self.De
        a = ops.linear_f32(x_t.view(B * Hs, self.A), model.action_in_proj.weight, model.action_in_proj.bias)
        pre = ops.linear_f32(a, sch.w_act, sch.tvec[step].contiguous())
        y = ops.linear_f32(ops.silu_f32(pre), model.action_time_mlp_out.weight, model.action_time_mlp_out.bias)
        ops.copy_rows(ops.cast(y, BF16).view(B, Hs, De), xs.view(B, self.Ss, De)[:, 1:])
        return pre

    def _pi0_state_rows(self, state):
        """pi0's suffix rows bf16 [B (Hs + 1), De] of one request with row 0 of every sample, the state token bf16(state_proj(state)),
        written: constant over the Euler steps (rows 1 .. Hs: `_pi0_suffix_embed`, every step)."""
        model, B, De = self.model, self.B, self.De
        xs = torch.empty((B * self.Ss, De), dtype=BF16, device=self.dev)
        s = ops.linear_f32(state.to(F32).contiguous(), model.state_proj.weight, model.state_proj.bias)
        ops.copy_rows(ops.cast(s, BF16).view(B, 1, De), xs.view(B, self.Ss, De)[:, :1])
        return xs

    def _denoise_step(self, x_t, step: int, sch, xs=None, tape: list | None = None):
        """One Euler step on the generic path (shapes the production stack was not built for) -> the velocity f32 [B, Hs, A].  Per layer:
        norm, three projection GEMMs into the static buffers, RoPE, attention, o_proj + residual, norm, GeGLU MLP + residual; then the
        final norm and action_out_proj.  The two model variants differ in data only:
          pi0.5: Hs rows per sample, embedded by action_in_proj; adaRMS norms with the step's rows of `sch.mods` / `sch.mf`; gated residuals;
          pi0:   Hs + 1 rows per sample in the request's `xs` (row 0, the state token, written once by `_run` and recomputed through the
                 layers every step, as the reference does; rows 1 .. Hs by `_pi0_suffix_embed`); plain RMSNorms, no gates;
                 action_out_proj reads the last Hs rows.
        `tape` (a guided step, `_denoiser_vjp`): the same launches, and what the reverse sweep needs is kept and appended per layer — the
        inputs of both norms with their rstd, the gates, g / u, the attention's rotated query rows, output rows and probabilities (all
        suffix rows of a sample); the final norm's input and rstd come last, with pi0's SiLU input `pre`.  pi0's plain norms then run
        as kai0_adarms_fwd over the constant modulation rows of `_guided_schedule` (the same arithmetic — x_hat (1 + w) + 0.0 — and it
        returns the rstd that kai0_rmsnorm's wrapper keeps to itself): `sch` must be that record."""
        model, ex = self.model, self.pe.gemma_expert.model
        B, P, Hs, Ss, De = self.B, self.P, self.Hs, self.Ss, self.De
        H, HD, S_ld = self.H, self.HD, self.S_ld
        NQ = H * HD
        ada = self.pi05
        taped = tape is not None
        inv_freq = self._inv_freq
        rows = slice(step * B, (step + 1) * B)
        pre = None
        if ada:
            a = ops.linear_f32(x_t.view(B * Hs, self.A), model.action_in_proj.weight, model.action_in_proj.bias)
            xs = ops.cast(a, BF16)
        else:
            pre = self._pi0_suffix_embed(x_t, step, sch, xs)

        def norm(x, ln, mod):  # -> (y, gate | None, rstd | None)
            if ada:
                return ops.adarms_fwd(x, mod[rows], x.shape[0] // B, ln.eps)  # (`rstd` is what the guided step's reverse sweep reads)
            if taped:
                y, _, rstd = ops.adarms_fwd(x, mod, x.shape[0] // B, ln.eps)
                return y, None, rstd
            return ops.rmsnorm(x, ln.weight, ln.eps), None, None

        for l, layer in enumerate(ex.layers):
            m1, m2 = sch.mods[l] if ada or taped else (None, None)
            x_in = xs
            hs, gate1, rstd1 = norm(xs, layer.input_layernorm, m1)
            at = layer.self_attn
            self._proj_into(hs, at.q_proj, self.q_buf, Ss, P, NQ)
            self._proj_into(hs, at.k_proj, self.k_cache[l], Ss, P, HD)
            self._proj_into(hs, at.v_proj, self.v_cache[l], Ss, P, HD)
            ops.rope_(self.q_buf[:, P : P + Ss], self.pos_suffix, inv_freq, HD)
            ops.rope_(self.k_cache[l][:, P : P + Ss], self.pos_suffix, inv_freq, HD)
            probs = self._attend(l, P, Ss, P + Ss, self.qcode, self.kcode, want_probs=tape is not None)
            if tape is not None:  # q_buf / att_buf are shared by the layers: this layer's suffix rows, compact [B Ss, H HD]
                q_rows = torch.empty((B * Ss, NQ), dtype=BF16, device=self.dev)
                att_rows = torch.empty((B * Ss, NQ), dtype=BF16, device=self.dev)
                ops.copy_rows(self.q_buf[:, P : P + Ss], q_rows.view(B, Ss, NQ))
                ops.copy_rows(self.att_buf[:, P : P + Ss], att_rows.view(B, Ss, NQ))
            xs = self._oproj(at.o_proj, Ss, P, residual=xs, gate=gate1)
            x_mid = xs
            hs, gate2, rstd2 = norm(xs, layer.post_attention_layernorm, m2)
            g = ops.linear_fwd(hs, layer.mlp.gate_proj.weight)
            u = ops.linear_fwd(hs, layer.mlp.up_proj.weight)
            h = ops.geglu_fwd(g, u, out=g if tape is None else None)  # in place, unless the sweep's kai0_geglu_bwd reads g
            xs = ops.linear_fwd(h, layer.mlp.down_proj.weight, residual=xs, gate=gate2, gate_rpb=Hs if ada else 0)
            if tape is not None:
                tape.append((x_in, rstd1, gate1, q_rows, att_rows, probs, x_mid, rstd2, gate2, g, u))
        out, _, rstd_f = norm(xs, ex.norm, sch.mf if ada or taped else None)
        if tape is not None:
            tape.append((xs, rstd_f, pre))
        if Ss != Hs:  # pi0: the action rows of every sample, compact
            act = torch.empty((B * Hs, De), dtype=BF16, device=self.dev)
            ops.copy_rows(out.view(B, Ss, De)[:, Ss - Hs :], act.view(B, Hs, De))
            out = act
        v = ops.linear_f32(ops.cast(out, F32), model.action_out_proj.weight, model.action_out_proj.bias)
        return v.view(B, Hs, self.A)

    # ------------------------------------------------------------------------------- real-time chunking (guided sampling)
    def _dgrad(self, dy, w, *, a_map=None, into=None):
        """dx [M, K] = dy [M, N] @ w [N, K] (ops.LinearFn.backward's dgrad form); `into`: dx is added to it (one bf16 rounding).
        a_map: dy's rows addressed through kai0_gemm_desc's row remap."""
        # (not ops.dgrad: this is the NN form inside a captured graph, and must never start transposing weights at 4096 rows)
        N, K = w.shape
        M = self.B * self.Ss
        if into is None:
            dx = torch.empty((M, K), dtype=BF16, device=self.dev)
            gemm(dy, w, dx, M=M, N=K, K=N, a_kc=True, b_kc=False, lda=N, ldb=K, ldc=K, a_map=a_map, split_k=pick_split_k(M, K, N))
            return dx
        gemm(dy, w, into, M=M, N=K, K=N, a_kc=True, b_kc=False, lda=N, ldb=K, ldc=K, a_map=a_map, accumulate=True, split_k=1)
        return into

    def _adarms_bwd(self, dy, x, mod, rstd, dres):
        """dx of y = adaRMS(x, mod) (+ dres, the residual branch's gradient, added inside the kernel); the modulation's gradient is dropped."""
        return ops.adarms_bwd(dy, x, mod, rstd, x.shape[0] // self.B, dres=dres)[0]

    def _gated_bwd(self, dout, gate):
        """d(y) of out = x + y * gate[b]: bf16(dout * gate[b]).  The gate's gradient (the only reader of y) is dropped: `dout` stands in for y."""
        return ops.gated_bwd(dout, dout, gate, dout.shape[0] // self.B)[0]

    def _denoiser_vjp(self, cot, tape, step: int, sch):
        """(dv / dx_t)^T cot for the step `_denoise_step(..., tape)` just ran: cot f32 [B Hs, A] -> f32 [B Hs, A]; sch: the record of
        `_guided_schedule`.  An explicit reverse sweep over the C entry points of the training backward (the arithmetic and rounding
        points of autograd over the bf16 model), called directly: not through the autograd shims, which would write weight gradients
        into a trainer's buffers (ops._grad_dst).  Only the path x_t -> v is differentiated; weights, modulations, the time vectors and
        the prefix K / V are constants.  Attention: dS and dQ for the Ss H folded suffix rows against all P + Ss keys in one launch
        (kai0_attn_bwd_dq over the stored probabilities), dK / dV for the suffix key rows only, as two TN GEMMs over the key columns
        [P, P + Ss) of dS and P (widened to 16-byte boundaries).
        pi0: the sweep carries all Ss = Hs + 1 rows of a sample.  The state row's cotangent starts at zero (action_out_proj reads the
        action rows), picks up the state KEY's dK / dV — column P of the window, which therefore starts where pi0.5's does — and is
        never read: every launch but the attention is row-wise, and the state query (mask code 1) has probability exactly 0 on the
        action keys [P + 1, P + Ss), so nothing of that row reaches an action row's dK / dV / dQ.  The norms' backward takes the
        constant modulation rows, the ungated residuals hand their cotangent on unchanged, and behind the first layer the suffix
        embedding is undone in exact f32: action_time_mlp_out^T, silu'(pre), the action half of action_time_mlp_in^T, action_in_proj^T
        (the time half and the biases take no gradient)."""
        model = self.model
        B, P, Hs, Ss, De, A = self.B, self.P, self.Hs, self.Ss, self.De, self.A
        H, HD, S_ld = self.H, self.HD, self.S_ld
        NQ, M, R = H * HD, B * Ss, Ss * H
        dev = self.dev
        ada = self.pi05
        rows = slice(step * B, (step + 1) * B)
        mods = [(a[rows], b[rows]) for a, b in sch.mods] if ada else sch.mods
        mf = sch.mf[rows] if ada else sch.mf
        layers = self.pe.gemma_expert.model.layers
        # action_out_proj^T: d(out32)[m, k] = sum_a cot[m, a] w_out[a, k]; the f32 <- bf16 cast hands its gradient on rounded to bf16
        d32 = torch.empty((B * Hs, De), dtype=F32, device=dev)
        ops.gemm_f32(cot, A, 1, model.action_out_proj.weight, De, 1, d32, B * Hs, De, A)
        dout = ops.cast(d32, BF16)
        if Ss != Hs:  # pi0: action_out_proj read the last Hs rows of every sample; the state row's output has no reader
            act = dout
            dout = torch.zeros((M, De), dtype=BF16, device=dev)
            ops.copy_rows(act.view(B, Hs, De), dout.view(B, Ss, De)[:, Ss - Hs :])
        x_last, rstd_f, pre = tape[-1]
        dxs = self._adarms_bwd(dout, x_last, mf, rstd_f, None)
        c0 = P // 8 * 8  # the suffix key columns, from a 16-byte boundary of the probability rows
        kw, koff = round_up(P + Ss - c0, 8), P - c0
        for l in range(len(layers) - 1, -1, -1):
            layer = layers[l]
            x_in, rstd1, gate1, q_rows, att_rows, probs, x_mid, rstd2, gate2, g, u = tape[l]
            at, mlp = layer.self_attn, layer.mlp
            # xs = x_mid + down(geglu(gate(hs2), up(hs2))) * gate2,  hs2 = adaRMS(x_mid, m2)   (pi0: no gate)
            dh = self._dgrad(self._gated_bwd(dxs, gate2) if ada else dxs, mlp.down_proj.weight)
            dg, du = ops.geglu_bwd(dh, g, u)
            dhs = self._dgrad(du, mlp.up_proj.weight, into=self._dgrad(dg, mlp.gate_proj.weight))
            dxs = self._adarms_bwd(dhs, x_mid, mods[l][1], rstd2, dxs)
            # x_mid = x_in + o_proj(attention(q, k, v)) * gate1,  q | k | v = rope(proj(adaRMS(x_in, m1)))
            datt = self._dgrad(self._gated_bwd(dxs, gate1) if ada else dxs, at.o_proj.weight)
            dS, dq = ops.attn_bwd_dq_stored(datt, att_rows, probs, self.k_cache[l], self.v_cache[l], batch=B, rows=R, Sk=P + Ss, HD=HD, ldo=HD,
                                            ldk=HD, ldv=HD, ldp=S_ld, sO=R * HD, sK=S_ld * HD, sV=S_ld * HD, sP=R * S_ld, scale=HD**-0.5)
            dkv = torch.empty((2, B, kw, HD), dtype=BF16, device=dev)
            for dst, a_t, b_t in ((dkv[0], dS, q_rows), (dkv[1], probs, datt)):  # dK = dS^T Q, dV = P^T dO over the suffix key columns
                gemm(a_t, b_t, dst, M=kw, N=HD, K=R, a_kc=False, b_kc=False, lda=S_ld, ldb=HD, ldc=HD, batch=B, sA=(R * S_ld, 0),
                     sB=(R * HD, 0), sC=(kw * HD, 0), a_off_elems=c0)
            ops.rope_(dq.view(B, Ss, NQ), self.pos_suffix, self._inv_freq, HD, inverse=True)
            ops.rope_(dkv[0][:, koff : koff + Ss], self.pos_suffix, self._inv_freq, HD, inverse=True)
            dhs = self._dgrad(dq, at.q_proj.weight)
            self._dgrad(dkv[0], at.k_proj.weight, a_map=(Ss, kw, koff), into=dhs)
            self._dgrad(dkv[1], at.v_proj.weight, a_map=(Ss, kw, koff), into=dhs)
            dxs = self._adarms_bwd(dhs, x_in, mods[l][0], rstd1, dxs)
        jte = torch.empty((B * Hs, A), dtype=F32, device=dev)
        if ada:  # xs = bf16(action_in_proj(x_t)): action_in_proj^T of the gradient as f32
            ops.gemm_f32(ops.cast(dxs, F32), De, 1, model.action_in_proj.weight, A, 1, jte, M, A, De)
            return jte
        # pi0: rows 1 .. Hs of xs = bf16(y),  y = W_out silu(pre) + b_out,  pre = w_act a + tvec[step],  a = action_in_proj(x_t)
        Ma = B * Hs
        dy = torch.empty((Ma, De), dtype=BF16, device=dev)
        ops.copy_rows(dxs.view(B, Ss, De)[:, Ss - Hs :], dy.view(B, Hs, De))
        dh = torch.empty((Ma, De), dtype=F32, device=dev)
        ops.gemm_f32(ops.cast(dy, F32), De, 1, model.action_time_mlp_out.weight, De, 1, dh, Ma, De, De)
        dpre = ops.silu_bwd_f32(dh, pre)
        da = torch.empty_like(dh)
        ops.gemm_f32(dpre, De, 1, sch.w_act, De, 1, da, Ma, De, De)
        ops.gemm_f32(da, De, 1, model.action_in_proj.weight, A, 1, jte, Ma, A, De)
        return jte

    def _seams_pi05(self, x2, sch, rope, n: int, dt: float):
        """pi0.5's Euler loop on the production stack.  Step seams in one launch each (kai0_denoise_glue): [final adaRMS ->
        action_out_proj -> Euler update] of step s and [action_in_proj -> bf16 + the rows' sums of squares] of step s + 1."""
        model, B, Hs, De = self.model, self.B, self.Hs, self.De
        M = B * Hs
        win, bin_ = model.action_in_proj.weight, model.action_in_proj.bias
        wout, bout = model.action_out_proj.weight, model.action_out_proj.bias
        eps = self.pe.gemma_expert.model.norm.eps
        xs = torch.empty((M, De), dtype=BF16, device=self.dev)
        sq = torch.empty((1, M), dtype=F32, device=self.dev)
        ops.denoise_glue(x2, w_in=win, b_in=bin_, xs_next=xs, rowsq_next=sq)
        last = None
        for step in range(n + 1):
            if step > 0:  # the seam behind step - 1 (and in front of `step`, if there is one)
                more = step < n
                xs = torch.empty((M, De), dtype=BF16, device=self.dev) if more else None
                sq = torch.empty((1, M), dtype=F32, device=self.dev) if more else None
                r_prev = slice((step - 1) * B, step * B)
                ops.denoise_glue(x2, xs=last, mod=sch.mf[r_prev], mod_ld=sch.mod_ld, rows_per_batch=Hs, eps=eps, w_out=wout, b_out=bout,
                                 dt=dt, w_in=win if more else None, b_in=bin_ if more else None, xs_next=xs, rowsq_next=sq)
            if step < n:
                last = self._expert_stack_folded(xs, sq, step, sch, rope)

    def _seams_pi0(self, x2, sch, rope, n: int, dt: float, state):
        """pi0's Euler loop on the production stack.  One suffix buffer xs [B (Hs + 1), De] + its sums of squares [De / 16, B (Hs + 1)]
        for all steps: row 0 of every sample = bf16(state_proj(state)), written once per request (kai0_denoise_glue_rows' opening half
        with w_in = state_proj); rows 1 .. Hs by `ops.pi0_suffix_embed` at the start of every step.  The seam behind a step is
        kai0_denoise_glue_rows' closing half on the action rows: the final plain RMSNorm as the constant modulation row `_mod_final`,
        action_out_proj, the Euler update of x_t.  The state token's layers are recomputed every step, as the reference does."""
        model, B, Hs, Ss, De = self.model, self.B, self.Hs, self.Ss, self.De
        xs = torch.empty((B * Ss, De), dtype=BF16, device=self.dev)
        sq = torch.zeros((De // 16, B * Ss), dtype=F32, device=self.dev)  # the state rows keep ONE partial (row 0 of sq), the rest 0
        ops.denoise_glue(state.to(F32).contiguous(), w_in=model.state_proj.weight, b_in=model.state_proj.bias, xs_next=xs, rowsq_next=sq,
                         row_map=(1, Ss, 0))
        ex_norm = self.pe.gemma_expert.model.norm
        w_a, b_a = model.action_in_proj.weight, model.action_in_proj.bias
        w_in, w_out, b_out = model.action_time_mlp_in.weight, model.action_time_mlp_out.weight, model.action_time_mlp_out.bias
        for step in range(n):
            ops.pi0_suffix_embed(x2, w_a, b_a, w_in, sch.tvec[step], w_out, b_out, xs, sq, Hs, Ss)
            last = self._expert_stack_folded(xs, sq, step, sch, rope)
            ops.denoise_glue(x2, xs=last, mod=self._mod_final, mod_ld=3 * De, rows_per_batch=B * Hs, eps=ex_norm.eps,
                             w_out=model.action_out_proj.weight, b_out=model.action_out_proj.bias, dt=dt, row_map=(Hs, Ss, Ss - Hs))

    def _run(self, images, img_masks, lang_tokens, lang_masks, noise, num_steps: int, state=None):
        """One action chunk: the schedule's record, the prefix pass, the Euler loop (production stack or generic step), the content
        stamp.  Every launch goes to the current stream: this is what `sample_actions` captures."""
        if not self.pi05:
            if state is None and self._static_in is not None:
                state = self._static_in["state"]  # the captured request's (a stage timed on the static inputs)
            if state is None:
                raise ValueError("a pi0 engine needs the request's `state`")
        times = euler_times(num_steps)
        dt = float(np.float32(-1.0 / num_steps))
        sch = self._schedule(times)
        x_t = noise.clone().contiguous()
        self._prefix_pass(images, img_masks, lang_tokens, lang_masks)
        B, P, HD, S_ld = self.B, self.P, self.HD, self.S_ld
        if self.fast:
            rope = ops.rope_table(self.pos_suffix, self._inv_freq)
            # prefix value rows of every layer -> transposed cache, one launch
            ops.transpose_strided(self.v_all, self.vt_all, R=P, C=HD, src_ld=HD, dst_ld=S_ld, batch=self.L * B, src_bs=S_ld * HD,
                                  dst_bs=HD * S_ld)
            x2 = x_t.view(B * self.Hs, self.A)
            if self.pi05:
                self._seams_pi05(x2, sch, rope, len(times), dt)
            else:
                self._seams_pi0(x2, sch, rope, len(times), dt, state)
        else:
            xs = None if self.pi05 else self._pi0_state_rows(state)  # the state token, row 0 of every sample's suffix rows
            for step in range(len(times)):
                v_t = self._denoise_step(x_t, step, sch, xs)
                ops.euler_step_(x_t, v_t, dt)
        self._content_stamp()
        return x_t

    def _run_guided(self, images, img_masks, lang_tokens, lang_masks, noise, num_steps: int, max_guidance_weight: float, provided: int,
                    mask_delay: bool = False, state=None):  # fmt: skip
        """A real-time-chunking chunk (pi0_rtc.py:293-349; kai0_amd/rtc.py): the prefix pass and the schedule record of `_run`, then per
        Euler step ONE forward of the generic per-layer step that keeps what its reverse sweep needs (the linearisation point),
        kai0_rtc_error, the sweep `_denoiser_vjp`, kai0_rtc_update.  One stream; t, the guidance weight and dt are launch constants;
        the previous chunk, the prefix weights and the delay rows are read from the engine's static buffers `_g_prev` / `_g_w` /
        `_g_delay`.  mask_delay (`mask_prefix_delay`, :322-327): the denoiser is evaluated and linearised at x_t with the delay rows'
        provided columns overwritten by the previous chunk (kai0_rtc_overwrite), the error is taken there, and the update goes to the
        original x_t."""
        from . import rtc

        times = euler_times(num_steps)
        dt = float(np.float32(-1.0 / num_steps))
        sch = self._guided_schedule(times)
        gws = rtc.guidance_weights(times, max_guidance_weight)
        x_t = noise.clone().contiguous()
        self._prefix_pass(images, img_masks, lang_tokens, lang_masks)
        xs = None if self.pi05 else self._pi0_state_rows(state)
        M = self.B * self.Hs
        for step, (t, g) in enumerate(zip(times, gws, strict=True)):
            tape = []
            x_den = ops.rtc_overwrite(x_t, self._g_prev, self._g_delay, provided) if mask_delay else x_t
            v_t = self._denoise_step(x_den, step, sch, xs, tape=tape)
            err = ops.rtc_error(x_den, v_t, self._g_prev, self._g_w, provided, t)
            jte = self._denoiser_vjp(err.view(M, self.A), tape, step, sch)
            ops.rtc_update_(x_t, v_t, err, jte, t, g, dt)
        self._content_stamp()
        return x_t

    @torch.no_grad()
    def denoiser_vjp(self, images, img_masks, lang_tokens, lang_masks, x_t, cotangent, num_steps: int, step: int, state=None):
        """The guided loop's primitive on its own (tests, tools): the prefix pass, then at `x_t` and the time of Euler step `step` the
        velocity v and (dv / dx_t)^T cotangent, both f32 [B, Hs, A].  Eager launches.  `state`: as `sample_actions` takes it (pi0)."""
        if not self.pi05 and state is None:
            raise ValueError("a pi0 engine needs the request's `state`")
        sch = self._guided_schedule(euler_times(num_steps))
        self._prefix_pass(images, img_masks, lang_tokens, lang_masks)
        xs = None if self.pi05 else self._pi0_state_rows(state)
        tape = []
        x_t = x_t.to(F32).contiguous()
        v_t = self._denoise_step(x_t, step, sch, xs, tape=tape)
        jte = self._denoiser_vjp(cotangent.to(F32).contiguous().view(self.B * self.Hs, self.A), tape, step, sch)
        return v_t, jte.view(self.B, self.Hs, self.A)

    @torch.no_grad()
    def sample_actions_guided(self, images, img_masks, lang_tokens, lang_masks, noise, guidance, num_steps: int = 10, state=None):
        """`sample_actions` steered towards the previous chunk (`guidance`: kai0_amd.rtc.Guidance, resolved on the host).  Captured into
        a hipGraph of its own, keyed on what is baked into its launches (num_steps, max_guidance_weight, provided, and whether
        `mask_prefix_delay` overwrites — the delay itself is data: the rows of `_g_delay`); the unguided graph and its static buffers
        are not touched.  KAI0_INFER_GRAPH=0 (or a refused capture) runs the same launches eagerly.  `state`: as `sample_actions`."""
        if self.pi05:
            state = None
        elif state is None:
            raise ValueError("a pi0 engine needs the request's `state`")
        B, Hs, A = self.B, self.Hs, self.A
        if guidance.prev.shape != (B, Hs, A) or guidance.weights.shape != (Hs,):
            raise ValueError(f"guidance for a [{B}, {Hs}, {A}] chunk expected, got prev {guidance.prev.shape}, weights {guidance.weights.shape}")
        if self._g_prev is None:
            self._g_prev = torch.zeros((B, Hs, A), dtype=F32, device=self.dev)
            self._g_w = torch.zeros((Hs,), dtype=F32, device=self.dev)
            self._g_delay = torch.zeros((Hs,), dtype=F32, device=self.dev)
        self._g_prev.copy_(torch.from_numpy(guidance.prev))
        self._g_w.copy_(torch.from_numpy(guidance.weights))
        mask_delay = bool(guidance.mask_prefix_delay) and guidance.provided > 0  # (:323)
        if mask_delay:
            self._g_delay.copy_(torch.from_numpy(guidance.delay_rows))
        key = (num_steps, float(guidance.max_guidance_weight), int(guidance.provided), mask_delay)
        args = (images, img_masks, lang_tokens, lang_masks, noise)
        if self.use_graph and self._g_graph_key != key:
            cap = _Capture(*args, state)
            self._g_cap, self._g_graph_key = None, key  # (a refused capture is not tried again for this key)
            try:
                cap.capture(lambda im, mk, tok, lm, nz, st: self._run_guided(im, mk, tok, lm, nz, *key, st))
                self._g_cap = cap
            except Exception as e:  # noqa: BLE001 - capture problems must not take serving down
                logger.warning("hipGraph capture of the guided chunk failed (%s); running eager HIP launches", e)
        if not self.use_graph or self._g_cap is None:
            return self._run_guided(*args, *key, state)
        self._g_cap.replay(*args, state)
        return self._g_cap.out.clone()

    # -------------------------------------------------------------------------------------------------- API
    @torch.no_grad()
    def sample_actions(self, images, img_masks, lang_tokens, lang_masks, noise, num_steps: int = 10, state=None):
        """`state`: the request's robot state f32 [B, action_dim] — a model input of pi0 (ignored by pi0.5, whose state is in the prompt)."""
        if self.pi05:
            state = None
        args = (images, img_masks, lang_tokens, lang_masks, noise)
        if self.use_graph and (self._cap is None or self._graph_steps != num_steps):
            cap = _Capture(*args, state)
            try:
                cap.capture(lambda im, mk, tok, lm, nz, st: self._run(im, mk, tok, lm, nz, num_steps, st))
                self._cap, self._graph_steps = cap, num_steps
            except Exception as e:  # noqa: BLE001 - capture problems must not take serving down
                logger.warning("hipGraph capture failed (%s); running eager HIP launches", e)
                self._cap = None
                self.use_graph = False
        if not self.use_graph:  # switched off, or capture refused: eager HIP launches
            return self._run(*args, num_steps, state)
        self._cap.replay(*args, state)
        return self._cap.out.clone()

    @torch.no_grad()
    def replay_then_verify(self, images, img_masks, lang_tokens, lang_masks, noise, num_steps: int, state=None):
        """The serving fast path: queue the captured chunk first, THEN check that the weights are still the ones the engine was built
        from (the check is host work; the chunk only writes engine-owned buffers).  Returns the chunk, or None when there is no graph for
        this schedule yet or the weights changed (the queued result is then dropped: the caller rebuilds the engine and runs again)."""
        if not self.use_graph or self._cap is None or self._graph_steps != num_steps:
            return None
        self._cap.replay(images, img_masks, lang_tokens, lang_masks, noise, None if self.pi05 else state)
        if not self.weights_unchanged():
            return None
        return self._cap.out.clone()


class _Capture:
    """Static copies of one request's inputs, a hipGraph recorded over them, and the tensor that graph writes its chunk to."""

    def __init__(self, images, img_masks, lang_tokens, lang_masks, noise, state=None):
        self.inputs = {
            "images": [im.clone().contiguous() for im in images],
            "img_masks": [m.clone() for m in img_masks],
            "lang_tokens": lang_tokens.clone().contiguous(),
            "lang_masks": lang_masks.clone().contiguous(),
            "noise": noise.clone().contiguous(),
            "state": state.to(F32).clone().contiguous() if state is not None else None,  # pi0: a static buffer inside the graph
        }
        self.graph = self.out = None

    def capture(self, run):
        """Record run(images, img_masks, lang_tokens, lang_masks, noise, state) -> chunk over the static copies.  Raises what the
        warm-up or the capture raises: what a refused capture means is the caller's business."""
        args = tuple(self.inputs.values())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up on a side stream, as graph capture requires
            run(*args)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run(*args)
        self.graph, self.out = graph, out

    def replay(self, images, img_masks, lang_tokens, lang_masks, noise, state=None):
        """Copy a request into the static buffers and queue the graph: the chunk lands in `out`."""
        si = self.inputs
        if si["state"] is not None:
            si["state"].copy_(state)
        for dst, src in zip(si["images"], images, strict=True):
            dst.copy_(src)
        for dst, src in zip(si["img_masks"], img_masks, strict=True):
            dst.copy_(src)
        si["lang_tokens"].copy_(lang_tokens)
        si["lang_masks"].copy_(lang_masks)
        si["noise"].copy_(noise)
        self.graph.replay()
