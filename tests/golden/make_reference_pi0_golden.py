"""Golden vectors of the pi0 branch (`pi05=False`) produced by EXECUTING THE REFERENCE'S OWN CODE on the tiny configuration.

Same method as make_reference_e2e_golden.py (definitions lifted out of the reference checkout with `ast`, nothing copied; the whole
path assembled from reference pieces on stub `self` objects), with the pi0 switches: `pol.pi05 = False`, a NON-adaptive expert
(GemmaRMSNorm without `cond_dim`, `use_adarms=False`), the heads `state_proj` / `action_time_mlp_in` / `action_time_mlp_out`.

Weights: the pi0.5 oracle's synthetic weights for every key pi0 shares; the pi0-only tensors (the three heads, the expert's plain
norm weights) from an explicit torch.Generator seed — they are stored in the fixture.  Inputs: the oracle's synthetic batch.
Stored: the reference's loss tensor, 10-step chunk, suffix embeddings / pad / att, gradients of mean(loss) for a spread of parameters,
and (metadata) the full list of state-dict keys with shapes and dtypes, and the noise floor — rel-L2 between the reference run with
bf16 storage and with f32 storage of the same weight values.

    python tests/golden/make_reference_pi0_golden.py      # build container only; needs the reference checkout
"""
import functools
import json
import logging
import os
import sys
import types
import typing

import torch
from safetensors.torch import save_file
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_reference_blocks_golden as B  # noqa: E402  (lift / lift_method / base_ns; rewrites the block fixture with the same bytes)
import pi0_restatement as R  # noqa: E402
from tiny import tiny_cfgs  # noqa: E402

from oracle import pi0_oracle as O  # noqa: E402

REF = B.REF
BF = torch.bfloat16
STD = 0.05  # matrices' std: the pi0.5 fixture's 0.08 gives a floor of 6.1e-3 (loss) / 2.1e-3 (chunk), above half the bounds; lowered as far as needed
PI0_SEED = 20240
LOSS_BOUND, CHUNK_BOUND = 1e-2, 3e-3  # tests/test_model_gpu.py's rel-L2 bounds
ident = lambda f: f  # noqa: E731


class Out:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class StubCache:  # transformers DynamicCache, the two calls the reference makes
    def __init__(self):
        self.k, self.v = [], []

    def get_seq_length(self, layer_idx=0):
        return self.k[0].shape[2] if self.k else 0

    def update(self, k, v, layer_idx, cache_kwargs=None):
        if layer_idx == len(self.k):
            self.k.append(k)
            self.v.append(v)
        else:
            self.k[layer_idx] = torch.cat([self.k[layer_idx], k], dim=2)
            self.v[layer_idx] = torch.cat([self.v[layer_idx], v], dim=2)
        return self.k[layer_idx], self.v[layer_idx]

    def __getitem__(self, i):
        return self.k[i], self.v[i]


def assign(module, sd, prefix):
    names = {n for n, _ in module.named_parameters()}
    got = {k[len(prefix):] for k in sd if k.startswith(prefix)}
    assert names <= got, (prefix, names - got)
    for n, p in module.named_parameters():
        p.data = sd[prefix + n].clone()  # keeps the stored dtype


_, ocfg05 = tiny_cfgs()
ocfg = R.pi0_cfg(ocfg05)
restated = R.build_restated(ocfg05, R.seeded_pi0_only(R.RestatedPI0(ocfg), PI0_SEED, STD), STD)
SD = {k: v.detach().clone() for k, v in restated.state_dict().items()}
PI0_ONLY = {k: SD[k] for k in R.pi0_only_keys(SD)}
obs, actions, noise, time = O.synthetic_batch(ocfg, 2, seed=0)
vlm, exp, sc = O.get_gemma_config("dummy"), O.get_gemma_config("dummy"), ocfg.siglip
PWE = "paligemma_with_expert."


def build_reference(sd, bf16: bool):
    """The reference's pi0 policy over lifted definitions with the weights `sd` -> (pol, {state-dict key: parameter})."""
    sns = B.base_ns()
    sns.update({"can_return_tuple": ident, "auto_docstring": ident, "BaseModelOutput": Out, "BaseModelOutputWithPooling": Out,
                "torch_int": int, "SiglipConfig": typing.Any, "PaliGemmaConfig": typing.Any})  # fmt: skip
    B.lift(f"{REF}/transformers_replace/models/siglip/modeling_siglip.py",
           ["eager_attention_forward", "SiglipAttention", "SiglipMLP", "SiglipEncoderLayer", "SiglipVisionEmbeddings", "SiglipEncoder",
            "SiglipVisionTransformer"], sns)  # fmt: skip
    scfg = types.SimpleNamespace(hidden_size=sc.hidden_size, num_hidden_layers=sc.num_layers, num_attention_heads=sc.num_heads,
                                 intermediate_size=sc.intermediate_size, patch_size=sc.patch_size, image_size=sc.image_size,
                                 num_channels=3, layer_norm_eps=sc.layer_norm_eps, hidden_act="gelu_pytorch_tanh",
                                 attention_dropout=0.0, _attn_implementation="eager", vision_use_head=False, output_attentions=False,
                                 output_hidden_states=False, projection_dim=sc.projection_dim)  # fmt: skip
    vt = sns["SiglipVisionTransformer"](scfg).eval()
    assign(vt, sd, PWE + "paligemma.model.vision_tower.vision_model.")
    pns = B.base_ns()
    pns.update({"PaliGemmaConfig": typing.Any, "can_return_tuple": ident, "auto_docstring": ident})
    B.lift(f"{REF}/transformers_replace/models/paligemma/modeling_paligemma.py", ["PaliGemmaMultiModalProjector"], pns)
    proj = pns["PaliGemmaMultiModalProjector"](types.SimpleNamespace(vision_config=scfg)).eval()
    assign(proj, sd, PWE + "paligemma.model.multi_modal_projector.")
    get_image_features = B.lift_method(f"{REF}/transformers_replace/models/paligemma/modeling_paligemma.py", "PaliGemmaModel",
                                       "get_image_features", pns)
    gns = B.base_ns()
    gns.update({"dynamic_rope_update": ident, "can_return_tuple": ident, "auto_docstring": ident, "ROPE_INIT_FUNCTIONS": {},
                "DynamicCache": StubCache, "create_causal_mask": lambda **kw: kw["attention_mask"], "BaseModelOutputWithPast": Out,
                "logger": logging.getLogger("ref")})  # fmt: skip
    B.lift(f"{REF}/transformers_replace/models/gemma/modeling_gemma.py",
           ["GemmaRMSNorm", "GemmaMLP", "GemmaRotaryEmbedding", "rotate_half", "apply_rotary_pos_emb", "repeat_kv", "_gated_residual",
            "eager_attention_forward", "GemmaAttention", "GemmaDecoderLayer"], gns)  # fmt: skip
    gemma_forward = B.lift_method(f"{REF}/transformers_replace/models/gemma/modeling_gemma.py", "GemmaModel", "forward", gns)

    def gemma_model(cfg, prefix, with_embed):  # both towers non-adaptive: use_adarms=[False, False] (pi0_pytorch.py:96)
        c = types.SimpleNamespace(hidden_size=cfg.width, num_attention_heads=cfg.num_heads, num_key_value_heads=cfg.num_kv_heads,
                                  head_dim=cfg.head_dim, attention_bias=False, attention_dropout=0.0, _attn_implementation="eager",
                                  intermediate_size=cfg.mlp_dim, hidden_act="gelu_pytorch_tanh", rms_norm_eps=1e-6,
                                  use_adarms=False, adarms_cond_dim=None, num_hidden_layers=cfg.depth,
                                  output_attentions=False, output_hidden_states=False, use_cache=False)  # fmt: skip
        layers = [gns["GemmaDecoderLayer"](c, i).eval() for i in range(cfg.depth)]
        for i, layer in enumerate(layers):
            assign(layer, sd, f"{prefix}layers.{i}.")
        norm = gns["GemmaRMSNorm"](cfg.width, cond_dim=None)
        assign(norm, sd, prefix + "norm.")
        Rot = gns["GemmaRotaryEmbedding"]
        rot = Rot.__new__(Rot)
        nn.Module.__init__(rot)
        inv = 1.0 / (10000.0 ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.int64).to(torch.float) / cfg.head_dim))
        # `.to(bfloat16)` on the module rounds the buffer; the f32-storage run keeps the same (rounded) VALUES, like the weights
        rot.register_buffer("inv_freq", inv.to(BF) if bf16 else inv.to(BF).float(), persistent=False)
        rot.attention_scaling = 1.0
        m = types.SimpleNamespace(config=c, gradient_checkpointing=False, training=False, layers=layers, norm=norm, rotary_emb=rot,
                                  embed_tokens=None)  # fmt: skip
        if with_embed:
            m.embed_tokens = nn.Embedding(ocfg.vocab_size, cfg.width)
            m.embed_tokens.weight.data = sd[prefix + "embed_tokens.weight"].clone()
        m.forward = functools.partial(gemma_forward, m)
        return m

    lm = gemma_model(vlm, PWE + "paligemma.model.language_model.", True)
    ex = gemma_model(exp, PWE + "gemma_expert.model.", False)
    jns = B.base_ns()
    import pytest

    jns.update({"pytest": pytest, "modeling_gemma": types.SimpleNamespace(
        **{k: gns[k] for k in ("apply_rotary_pos_emb", "eager_attention_forward", "_gated_residual")})})
    pwe = types.SimpleNamespace(training=False)
    pwe.paligemma = types.SimpleNamespace(
        language_model=lm,
        model=types.SimpleNamespace(language_model=lm, vision_tower=vt, multi_modal_projector=proj),
        config=types.SimpleNamespace(text_config=types.SimpleNamespace(num_hidden_layers=vlm.depth)))
    pwe.paligemma.model.get_image_features = functools.partial(get_image_features, pwe.paligemma.model)
    pwe.gemma_expert = types.SimpleNamespace(model=ex)
    for name in ("forward", "embed_image", "embed_language_tokens"):
        setattr(pwe, name, functools.partial(B.lift_method(f"{REF}/gemma_pytorch.py", "PaliGemmaWithExpertModel", name, jns), pwe))
    mns = B.base_ns()
    B.lift(f"{REF}/pi0_pytorch.py", ["get_safe_dtype", "create_sinusoidal_pos_embedding", "make_att_2d_masks"], mns)
    pol = types.SimpleNamespace(config=types.SimpleNamespace(action_horizon=ocfg.action_horizon, action_dim=ocfg.action_dim), pi05=False,
                                gradient_checkpointing_enabled=False, training=False, paligemma_with_expert=pwe)  # fmt: skip
    heads = {"action_in_proj": (ocfg.action_dim, exp.width), "action_out_proj": (exp.width, ocfg.action_dim),
             "state_proj": (ocfg.action_dim, exp.width), "action_time_mlp_in": (2 * exp.width, exp.width),
             "action_time_mlp_out": (exp.width, exp.width)}  # fmt: skip
    for head, (i, o) in heads.items():
        lin = nn.Linear(i, o)
        assign(lin, sd, head + ".")
        setattr(pol, head, lin)
    for name in ("_apply_checkpoint", "_prepare_attention_masks_4d", "embed_prefix", "embed_suffix", "denoise_step", "forward",
                 "sample_actions"):
        setattr(pol, name, functools.partial(B.lift_method(f"{REF}/pi0_pytorch.py", "PI0Pytorch", name, mns), pol))
    # preprocessing with train=False on images already at resolution is the identity (preprocessing_pytorch.py:20-173)
    pol._preprocess_observation = lambda o, train=True: (list(o.images.values()), list(o.image_masks.values()), o.tokenized_prompt,
                                                         o.tokenized_prompt_mask, o.state)  # fmt: skip
    params = {}
    for prefix, mod in ((PWE + "paligemma.model.vision_tower.vision_model.", vt), (PWE + "paligemma.model.multi_modal_projector.", proj),
                        *((h + ".", getattr(pol, h)) for h in heads)):
        params.update({prefix + n: p_ for n, p_ in mod.named_parameters()})
    for tower, prefix in ((lm, PWE + "paligemma.model.language_model."), (ex, PWE + "gemma_expert.model.")):
        for i, layer in enumerate(tower.layers):
            params.update({f"{prefix}layers.{i}.{n}": p_ for n, p_ in layer.named_parameters()})
        params.update({prefix + "norm." + n: p_ for n, p_ in tower.norm.named_parameters()})
    params[PWE + "paligemma.model.language_model.embed_tokens.weight"] = lm.embed_tokens.weight
    return pol, params


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


pol, ref_params = build_reference(SD, bf16=True)
with torch.no_grad():
    ref_loss = pol.forward(obs, actions, noise=noise, time=time)
    ref_actions = pol.sample_actions(torch.device("cpu"), obs, noise=noise.clone(), num_steps=10)
    t = time[:, None, None]
    suf, suf_pad, suf_att, suf_cond = pol.embed_suffix(obs.state, t * noise + (1 - t) * actions, time)
assert suf_cond is None
# the same weight VALUES stored in f32: what the bf16 choreography's own rounding costs (the floor under every bf16 implementation)
pol32, _ = build_reference({k: v.float() for k, v in SD.items()}, bf16=False)
with torch.no_grad():
    loss32 = pol32.forward(obs, actions, noise=noise, time=time)
    act32 = pol32.sample_actions(torch.device("cpu"), obs, noise=noise.clone(), num_steps=10)
floor_loss, floor_chunk = rel_l2(ref_loss, loss32), rel_l2(ref_actions, act32)
print(f"noise floor (bf16 vs f32 storage): loss rel-L2 {floor_loss:.3e} (bound/2 {LOSS_BOUND / 2:.1e}) | chunk rel-L2 {floor_chunk:.3e} "
      f"(bound/2 {CHUNK_BOUND / 2:.1e})")
assert floor_loss <= LOSS_BOUND / 2 and floor_chunk <= CHUNK_BOUND / 2, "lower STD"

GRAD_KEYS = ["state_proj.weight", "action_time_mlp_in.weight", "action_time_mlp_out.bias", "action_in_proj.weight", "action_out_proj.bias",
             PWE + "gemma_expert.model.layers.0.self_attn.q_proj.weight", PWE + "gemma_expert.model.layers.3.input_layernorm.weight",
             PWE + "gemma_expert.model.layers.1.post_attention_layernorm.weight", PWE + "gemma_expert.model.norm.weight",
             PWE + "gemma_expert.model.layers.2.mlp.down_proj.weight",
             PWE + "paligemma.model.language_model.layers.2.mlp.down_proj.weight",
             PWE + "paligemma.model.language_model.layers.0.input_layernorm.weight",
             PWE + "paligemma.model.vision_tower.vision_model.encoder.layers.1.mlp.fc1.weight",
             PWE + "paligemma.model.multi_modal_projector.linear.bias"]  # fmt: skip
for p_ in ref_params.values():
    p_.requires_grad_(True)
pol.forward(obs, actions, noise=noise, time=time).mean().backward()
ref_grads = {"grad." + k: ref_params[k].grad.detach().clone() for k in GRAD_KEYS}
no_grad = sorted(k for k, p_ in ref_params.items() if p_.grad is None or not bool(p_.grad.any()))

# ---- the restatement against the reference: expected 0.0 everywhere ------------------------------------------------------------
restated.zero_grad(set_to_none=True)
for p_ in restated.parameters():
    p_.requires_grad_(True)
restated(obs, actions, noise, time).mean().backward()
rg = dict(restated.named_parameters())
print("restatement vs reference gradients: max|d|", max(float((rg[k].grad - ref_grads["grad." + k]).abs().max()) for k in GRAD_KEYS))
with torch.no_grad():
    o_loss = restated(obs, actions, noise, time)
    o_act = restated.sample_actions(obs, noise.clone(), num_steps=10)
print("reference loss", tuple(ref_loss.shape), float(ref_loss.mean()), "| chunk", tuple(ref_actions.shape), float(ref_actions.abs().mean()),
      "| suffix", tuple(suf.shape), suf.dtype, "att", suf_att[0].tolist())
print("restatement vs reference: loss max|d|", float((o_loss - ref_loss).abs().max()), " chunk max|d|", float((o_act - ref_actions).abs().max()))

keys = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in SD.items()}
# the list is the REFERENCE's: every parameter of the lifted reference modules is in it with its shape and dtype, and nothing else but the
# two lm_heads the stubs do not instantiate (paligemma's tied to embed_tokens, the expert's dead one: gemma_pytorch.py:43-59)
heads = {PWE + "paligemma.lm_head.weight", PWE + "gemma_expert.lm_head.weight"}
assert set(ref_params) | heads == set(SD), set(ref_params) ^ set(SD)
assert all(list(p_.shape) == keys[k][0] and str(p_.dtype).replace("torch.", "") == keys[k][1] for k, p_ in ref_params.items())
save_file({**{k: v.contiguous() for k, v in ref_grads.items()}, **{"w." + k: v.contiguous() for k, v in PI0_ONLY.items()},
           "loss": ref_loss.contiguous(), "actions": ref_actions.contiguous(), "suffix": suf.contiguous(),
           "suffix_pad": suf_pad.contiguous(), "suffix_att": suf_att.contiguous().to(torch.float32),
           "noise": noise.contiguous(), "time": time.contiguous(), "in_actions": actions.contiguous()},
          os.path.join(HERE, "reference_pi0.safetensors"),
          # ONE metadata entry (a JSON document): the header's entries are written in hash order, several would make the file's bytes differ
          # from run to run
          metadata={"json": json.dumps({
              "config": "tests/tiny.tiny_cfgs() with pi05=False", "batch": "oracle.synthetic_batch(cfg, 2, seed=0)", "num_steps": 10,
              "weights": f"shared keys: oracle.synthetic_weights_(seed=0), matrices x{STD / 0.02:g} (std {STD}); pi0-only keys: "
                         f"tests/pi0_restatement.seeded_pi0_only(seed={PI0_SEED}, std={STD}), stored as w.<key>",
              "std": STD, "floor_loss_rel_l2": floor_loss, "floor_chunk_rel_l2": floor_chunk, "state_dict_keys": keys,
              "no_grad_keys": no_grad}, sort_keys=True)})  # fmt: skip
print("wrote reference_pi0.safetensors;", len(keys), "state-dict keys;", len(no_grad), "parameters without gradient")
