"""The oracle against the reference's own layers AT THE WIDTHS THE KERNELS RUN AT.

tests/test_reference_blocks_cpu.py pins the oracle to reference-executed vectors at toy widths (width 48-64, head_dim 16).
Here the reference's definitions, lifted from its source (tests/reflift.py), were executed at the real shapes of BASELINE.json's
model, with the weights and inputs of the oracle modules the `_*_case` functions below build from fixed seeds; their outputs are
committed (tests/golden/reference_realwidth.json, written by this file when run as a script next to a checkout of the
reference: per output its shape, dtype, the SHA-256 of its raw bf16 bytes and a fixed sample of its values; with them the thread
count, CPU kernel path and torch version they were computed with) and the oracle must reproduce them:

  * a whole action-expert GemmaDecoderLayer: width 1024, 8 query heads / 1 KV head of head_dim 256, MLP 4096, adaRMS
    conditioning, cached prefix K/V (modeling_gemma.py:344-384, 282-329);
  * a whole Gemma-2B prefix GemmaDecoderLayer: width 2048, MLP 16384;
  * a whole SiglipEncoderLayer: hidden 1152, 16 heads of head_dim 72, MLP 4304, 256 patch tokens (modeling_siglip.py:435-480);
  * the JOINT prefix + expert forward of PaliGemmaWithExpertModel (gemma_pytorch.py:126-279) with both towers at real width.

Same torch ops in the same order => the bf16 results must be bit-identical.  Which bits a bf16 CPU matmul produces depends on the
thread count (how the reduction is split) and on the CPU kernel path (torch.backends.cpu.get_cpu_capability()), so the record and
the test both run at THREADS threads; a host whose kernel path or torch differs from the record's computes other bits."""

import hashlib
import json
import os
import sys
import types

import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from oracle import pi0_oracle as O  # noqa: E402

BF = torch.bfloat16
GOLD = os.path.join(HERE, "golden", "reference_realwidth.json")
SAMPLE = 256  # values per output kept in the record (readable mismatches); the digest covers every element
THREADS = 1  # torch CPU threads of the recording and of the test: one, which every host has


def _conditions():
    return {"threads": torch.get_num_threads(), "cpu_capability": torch.backends.cpu.get_cpu_capability(), "torch": torch.__version__}


@pytest.fixture(scope="module")
def want():
    before = torch.get_num_threads()
    torch.set_num_threads(THREADS)
    with open(GOLD) as f:
        yield json.load(f)
    torch.set_num_threads(before)


def _digest(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).numpy().tobytes()).hexdigest()


def _sample(t):
    flat = t.reshape(-1)
    return flat[torch.randint(flat.numel(), (SAMPLE,), generator=torch.Generator().manual_seed(0))].float().tolist()


def _record_of(t):
    return {"shape": list(t.shape), "dtype": str(t.dtype), "sha256": _digest(t), "sample": _sample(t)}


def _assert_bit_identical(got, want, key):
    """got equals the recorded reference output bit for bit: shape, dtype, a sample of values, then every element's bits"""
    rec = want["outputs"][key]
    recorded = {k: want[k] for k in ("threads", "cpu_capability", "torch")}
    here = _conditions()
    why = (f"{key}: the oracle's bits differ from the reference's recorded ones (recorded under {recorded}, computed here under {here}"
           + ("; the conditions differ, which alone changes bf16 CPU matmul bits: a likely cause, not necessarily an oracle regression"
              if here != recorded else "") + ")")
    assert [list(got.shape), str(got.dtype)] == [rec["shape"], rec["dtype"]], why
    assert _sample(got) == rec["sample"], why
    assert _digest(got) == rec["sha256"], why
    assert float(got.float().abs().mean()) > 1e-2


def _rnd(g, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _set_params(g, mod, scale):
    for _, p in sorted(mod.named_parameters()):  # by name: the reference's modules have the oracle's parameter names
        p.data = _rnd(g, *p.shape, scale=(scale if p.dim() >= 2 else 0.1)).to(p.dtype)


def _selected_bf16(mod):
    """gemma_pytorch.py:63-83 on a single layer: everything bf16, the norms (incl. the adaRMS dense) back to f32"""
    mod.to(BF)
    for name, p in mod.named_parameters():
        if "layernorm" in name:
            p.data = p.data.to(torch.float32)


def _tables(g, B, S, HD=256):
    ang = _rnd(g, B, S, HD // 2, scale=3.0)
    return torch.cat([ang, ang], -1).cos().to(BF), torch.cat([ang, ang], -1).sin().to(BF)


def _decoder_case(kind):
    g = torch.Generator().manual_seed(7 if kind == "expert" else 8)
    adaptive = kind == "expert"
    width, mlp = (1024, 4096) if adaptive else (2048, 16384)
    B, S, Pk = 2, 24, (40 if adaptive else 0)
    cfg = O.GemmaCfg(width=width, depth=1, mlp_dim=mlp, num_heads=8, num_kv_heads=1, head_dim=256)
    model = O.GemmaModel(cfg, vocab=8, use_adarms=adaptive, with_embed=False)
    _set_params(g, model.layers[0], 0.03)
    _selected_bf16(model.layers[0])
    if adaptive:
        _set_params(g, model.norm, 0.03)
    h = _rnd(g, B, S, width, dtype=BF)
    cos, sin = _tables(g, B, S)
    past = [(_rnd(g, B, 1, Pk, 256, dtype=BF), _rnd(g, B, 1, Pk, 256, dtype=BF))] if adaptive else None
    allowed = torch.rand(B, 1, S, Pk + S, generator=g) > 0.25
    allowed[..., 0] = True
    mask = torch.where(allowed, 0.0, O.MASK_VALUE)
    cond = _rnd(g, B, width) if adaptive else None
    return types.SimpleNamespace(model=model, adaptive=adaptive, width=width, mlp=mlp, B=B, S=S, h=h, cos=cos, sin=sin, past=past,
                                 mask=mask, cond=cond)  # fmt: skip


@pytest.mark.parametrize("kind", ["expert", "prefix"])
def test_decoder_layer_at_real_width(want, kind):
    """the record: the reference layer's output through the oracle model's final norm (forward_single ends with it)"""
    c = _decoder_case(kind)
    real = O.rotary_cos_sin
    O.rotary_cos_sin = lambda inv, pos, dt: (c.cos, c.sin)  # the stored tables instead of position ids
    try:
        with torch.no_grad():
            got, _ = c.model.forward_single(c.h, c.mask, torch.zeros(c.B, c.S, dtype=torch.long), c.past, False, c.cond)
    finally:
        O.rotary_cos_sin = real
    assert got.dtype == BF
    _assert_bit_identical(got, want, f"decoder.{kind}")


def _siglip_case():
    g = torch.Generator().manual_seed(9)
    layer = O.SiglipEncoderLayer(O.SiglipCfg(num_layers=1))  # So400m/14 defaults: 1152 / 16 x 72 / 4304
    _set_params(g, layer, 0.03)
    layer.to(BF)
    return layer, _rnd(g, 2, 256, 1152, dtype=BF)


def test_siglip_layer_at_real_width(want):
    layer, x = _siglip_case()
    with torch.no_grad():
        got = layer(x)
    _assert_bit_identical(got, want, "siglip")


def _joint_case():
    """Gemma-2B width 2048 / 16384 next to the expert's 1024 / 4096, head_dim 256 MQA, padded prompt tokens, prefix-LM mask, one
    joint layer + the final norms; rotary from the bf16-rounded inv_freq."""
    g = torch.Generator().manual_seed(10)
    L = 1
    vlm = O.GemmaCfg(width=2048, depth=L, mlp_dim=16384, num_heads=8, num_kv_heads=1, head_dim=256)
    exp = O.GemmaCfg(width=1024, depth=L, mlp_dim=4096, num_heads=8, num_kv_heads=1, head_dim=256)
    sc = O.SiglipCfg(hidden_size=16, num_layers=1, num_heads=2, intermediate_size=32, patch_size=14, image_size=28, projection_dim=2048)
    model = O.PaliGemmaWithExpertModel(vlm, exp, use_adarms=[False, True], precision="bfloat16", vocab=16, sc=sc)
    olm, oex = model.paligemma.language_model, model.gemma_expert.model
    for layer in (*olm.layers, *oex.layers):
        _set_params(g, layer, 0.03)
    olm.norm.weight.data = _rnd(g, 2048, scale=0.3)
    _set_params(g, oex.norm, 0.03)
    olm.inv_freq = O.rope_inv_freq(256).to(BF)
    B, P_, S_ = 2, 48, 16
    pad = torch.ones(B, P_ + S_, dtype=torch.bool)
    pad[0, 40:48] = False
    att = torch.zeros(B, P_ + S_, dtype=torch.bool)
    att[:, P_] = True
    pos = torch.cumsum(pad, dim=1) - 1
    pre, suf = _rnd(g, B, P_, 2048, dtype=BF), _rnd(g, B, S_, 1024, dtype=BF)
    cond = _rnd(g, B, 1024)
    return types.SimpleNamespace(model=model, L=L, pad=pad, att=att, pos=pos, pre=pre, suf=suf, cond=cond)


def test_joint_forward_at_real_width(want):
    c = _joint_case()
    mask = torch.where(O.make_att_2d_masks(c.pad, c.att)[:, None, :, :], 0.0, O.MASK_VALUE)
    with torch.no_grad():
        (gp, gs), _ = c.model(mask, c.pos, None, [c.pre, c.suf], False, [None, c.cond])
    _assert_bit_identical(gp, want, "joint.prefix")
    _assert_bit_identical(gs, want, "joint.suffix")


# ---------------------------------------------------------------------------- recording the reference's outputs (script only)
def _gemma_cfg(width, mlp, adarms):
    return types.SimpleNamespace(hidden_size=width, num_attention_heads=8, num_key_value_heads=1, head_dim=256, attention_bias=False,
                                 attention_dropout=0.0, _attn_implementation="eager", intermediate_size=mlp,
                                 hidden_act="gelu_pytorch_tanh", rms_norm_eps=1e-6, use_adarms=adarms, adarms_cond_dim=width)  # fmt: skip


def _copy_layer(dst, src):
    """the oracle's weights into a reference module: same names, shapes and dtypes (to_bfloat16_for_selected_params chose the same)"""
    sd = dict(src.named_parameters())
    assert set(sd) == {n for n, _ in dst.named_parameters()}
    for n, p in dst.named_parameters():
        assert p.shape == sd[n].shape and p.dtype == sd[n].dtype, n
        p.data = sd[n].data.clone()


def _record(reflift):
    gem = reflift.lift(reflift.GEMMA_PY, ["GemmaRMSNorm", "GemmaMLP", "rotate_half", "apply_rotary_pos_emb", "repeat_kv",
                                          "_gated_residual", "eager_attention_forward", "GemmaAttention", "GemmaDecoderLayer"],
                       reflift.base_ns())  # fmt: skip
    sig = reflift.lift(reflift.SIGLIP_PY, ["eager_attention_forward", "SiglipAttention", "SiglipMLP", "SiglipEncoderLayer"],
                       reflift.base_ns())  # fmt: skip
    pi0 = reflift.lift(reflift.PI0_PY, ["make_att_2d_masks"], reflift.base_ns())
    out = {}
    with torch.no_grad():
        for kind in ("expert", "prefix"):
            c = _decoder_case(kind)
            layer = gem["GemmaDecoderLayer"](_gemma_cfg(c.width, c.mlp, c.adaptive), 0).eval()
            _selected_bf16(layer)
            _copy_layer(layer, c.model.layers[0])
            y = layer(c.h, attention_mask=c.mask, position_ids=None, past_key_value=c.past, use_cache=False,
                      position_embeddings=(c.cos, c.sin), adarms_cond=c.cond)[0]  # fmt: skip
            assert y.dtype == BF and float(y.float().abs().mean()) > 1e-2
            out[f"decoder.{kind}"], _ = c.model.norm(y, c.cond)

        layer, x = _siglip_case()
        scfg = types.SimpleNamespace(hidden_size=1152, num_attention_heads=16, intermediate_size=4304, layer_norm_eps=1e-6,
                                     hidden_act="gelu_pytorch_tanh", attention_dropout=0.0, _attn_implementation="eager")
        sl = sig["SiglipEncoderLayer"](scfg).eval().to(BF)
        _copy_layer(sl, layer)
        out["siglip"] = sl(x, attention_mask=None)[0]

        # PaliGemmaWithExpertModel.forward (both inputs) from the reference on a stub `self` holding reference layers; rotary from
        # the vendored GemmaRotaryEmbedding
        c = _joint_case()
        olm, oex = c.model.paligemma.language_model, c.model.gemma_expert.model
        gns = reflift.base_ns()
        gns.update({"dynamic_rope_update": (lambda f: f), "ROPE_INIT_FUNCTIONS": {}})
        reflift.lift(reflift.GEMMA_PY, ["GemmaRotaryEmbedding"], gns)
        Rot = gns["GemmaRotaryEmbedding"]
        rot = Rot.__new__(Rot)
        nn.Module.__init__(rot)
        rot.register_buffer("inv_freq", olm.inv_freq.clone(), persistent=False)
        rot.attention_scaling = 1.0
        vl = [gem["GemmaDecoderLayer"](_gemma_cfg(2048, 16384, False), i).eval() for i in range(c.L)]
        el = [gem["GemmaDecoderLayer"](_gemma_cfg(1024, 4096, True), i).eval() for i in range(c.L)]
        for refs, ours in ((vl, olm.layers), (el, oex.layers)):
            for r, o in zip(refs, ours, strict=True):
                _selected_bf16(r)
                _copy_layer(r, o)
        vnorm, enorm = gem["GemmaRMSNorm"](2048), gem["GemmaRMSNorm"](1024, cond_dim=1024)
        vnorm.weight.data = olm.norm.weight.data.clone()  # f32, as the oracle holds it (the reference initialises a bf16 zero vector)
        _copy_layer(enorm, oex.norm)
        lm = types.SimpleNamespace(layers=vl, norm=vnorm, rotary_emb=rot)
        ex = types.SimpleNamespace(layers=el, norm=enorm, gradient_checkpointing=False)
        stub = types.SimpleNamespace(
            paligemma=types.SimpleNamespace(language_model=lm, model=types.SimpleNamespace(language_model=lm),
                                            config=types.SimpleNamespace(text_config=types.SimpleNamespace(num_hidden_layers=c.L))),
            gemma_expert=types.SimpleNamespace(model=ex), training=False)  # fmt: skip
        jns = reflift.base_ns()
        jns.update({"pytest": pytest,
                    "modeling_gemma": types.SimpleNamespace(**{k: gem[k] for k in ("apply_rotary_pos_emb", "eager_attention_forward", "_gated_residual")})})  # fmt: skip
        joint = reflift.lift_method(reflift.GEMMA_PT_PY, "PaliGemmaWithExpertModel", "forward", jns)
        att2d = pi0["make_att_2d_masks"](c.pad, c.att)
        assert torch.equal(att2d, O.make_att_2d_masks(c.pad, c.att))  # the test builds the mask with the oracle's function
        mask = torch.where(att2d[:, None, :, :], 0.0, O.MASK_VALUE)
        (wp, ws), _ = joint(stub, attention_mask=mask, position_ids=c.pos, past_key_values=None, inputs_embeds=[c.pre, c.suf],
                            use_cache=False, adarms_cond=[None, c.cond])  # fmt: skip
        out["joint.prefix"], out["joint.suffix"] = wp, ws
    return out


if __name__ == "__main__":  # next to a checkout of the reference (tests/reflift.py): record its outputs
    import reflift

    assert reflift.available(), "needs the reference sources (tests/reflift.py)"
    torch.set_num_threads(THREADS)
    out = {**_conditions(), "outputs": {k: _record_of(v) for k, v in _record(reflift).items()}}
    with open(GOLD, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", GOLD, {k: v for k, v in out.items() if k != "outputs"}, {k: v["shape"] for k, v in out["outputs"].items()})
