"""LoRA on the host side, no GPU: the three LoRA variants of `get_config`, the freeze filter over the full-size model's names (meta
tensors), the sharding plan of the frozen model, the JAX <-> torch map of the ten adapter arrays per tower against the reference's
einsum equations (src/openpi/models/lora.py:54-85 `Einsum`, :144-148 `FeedForward._dot`), `merge_lora` against a float64 dense
construction, loading a base checkpoint into a LoRA model, and the unchanged names of models without adapters."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tiny import tiny_cfgs  # noqa: E402

from kai0_amd import convert, lora  # noqa: E402
from kai0_amd.config import GemmaConfig, LoRAConfig, Pi0Config, get_config  # noqa: E402

LLM = "PaliGemma/llm/"
PWE = "paligemma_with_expert."


def test_get_config_lora_variants():
    for plain, variant, rank in (("gemma_2b", "gemma_2b_lora", 16), ("gemma_300m", "gemma_300m_lora", 32), ("dummy", "dummy_lora", 8)):
        base, cfg = get_config(plain), get_config(variant)
        assert isinstance(cfg, GemmaConfig) and base.lora_configs == {} and set(cfg.lora_configs) == {"attn", "ffn"}
        assert (cfg.width, cfg.depth, cfg.mlp_dim, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim) == \
               (base.width, base.depth, base.mlp_dim, base.num_heads, base.num_kv_heads, base.head_dim)  # fmt: skip
        assert all(lc.rank == rank and not lc.rslora for lc in cfg.lora_configs.values())
    assert get_config("gemma_2b_lora").lora_configs["attn"].scaling_value == 1.0  # alpha 16 / rank 16 (gemma.py:96)
    assert get_config("gemma_300m_lora").lora_configs["ffn"].scaling_value == 1.0  # alpha 32 / rank 32 (gemma.py:107)
    assert get_config("dummy_lora").lora_configs["attn"].scaling_value == 2.0
    assert LoRAConfig(rank=16, alpha=8.0).scaling_value == 0.5
    assert LoRAConfig(rank=16, alpha=8.0, rslora=True).scaling_value == 2.0  # alpha / sqrt(rank), lora.py:30
    assert LoRAConfig(rank=4).scaling_value == 0.25 and LoRAConfig(rank=4).init_std == 0.01
    with pytest.raises(ValueError):
        get_config("gemma_7b_lora")


def _meta_model(pv, ev, pi05=True):
    from kai0_amd.model import PI0Pytorch

    with torch.device("meta"):
        model = PI0Pytorch(Pi0Config(paligemma_variant=pv, action_expert_variant=ev, pi05=pi05))
    model.paligemma_with_expert.to_bfloat16_for_selected_params("bfloat16")
    return model


def _adapter_elements(cfg: GemmaConfig) -> int:
    """lora.py:48-52 and :113-120 summed over a tower, from the configuration alone."""
    N, K, H, D, F = cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.width, cfg.mlp_dim
    ra, rf = cfg.lora_configs["attn"].rank, cfg.lora_configs["ffn"].rank
    attn = (N * D * ra + N * ra * H) + 2 * (K * D * ra + K * ra * H) + (N * H * ra + N * ra * D)
    ffn = 2 * (D * rf + rf * F) + (F * rf + rf * D)
    return cfg.depth * (attn + ffn)


CASES = [("gemma_2b_lora", "gemma_300m_lora"), ("gemma_2b_lora", "gemma_300m"), ("gemma_2b", "gemma_300m_lora")]


@pytest.mark.parametrize("pv,ev", CASES)
def test_freeze_filter_name_table_at_full_size(pv, ev):
    model = _meta_model(pv, ev)
    f = Pi0Config(paligemma_variant=pv, action_expert_variant=ev).get_freeze_filter()
    lm, ex = PWE + "paligemma.model.language_model.", PWE + "gemma_expert."
    # pi0_config.py:86-100: both towers / PaliGemma only (the expert stays trainable) / expert only
    frozen_lm, frozen_ex = "lora" in pv, "lora" in ev
    n_adapters = 0
    for name, _ in model.named_parameters(remove_duplicate=False):
        if ".lora_" in name:
            n_adapters += 1
            assert not f(name), name  # `.*lora.*` is never frozen
        elif name.startswith(lm) or name.startswith(PWE + "paligemma.lm_head."):
            assert f(name) == frozen_lm, name  # embedding, norms, projections, MLP, the tied head
        elif name.startswith(ex):
            assert f(name) == frozen_ex, name  # incl. the adaRMS `dense` layers, the final norm and the dead lm_head
        else:
            assert not f(name), name  # SigLIP, the projector, action / time heads
    towers = [t for t, v in (("p", pv), ("e", ev)) if "lora" in v]
    assert n_adapters == 18 * 14 * len(towers)
    for probe in ("embed_tokens.weight", "layers.3.input_layernorm.weight", "norm.weight", "layers.17.mlp.down_proj.weight"):
        assert f(lm + probe) == frozen_lm
    for probe in ("model.layers.0.input_layernorm.dense.weight", "model.norm.dense.bias", "lm_head.weight", "model.layers.5.self_attn.q_proj.weight"):
        assert f(ex + probe) == frozen_ex
    assert not f("action_in_proj.weight") and not f("time_mlp_out.bias") and not f(PWE + "paligemma.model.multi_modal_projector.linear.weight")
    assert not f(PWE + "paligemma.model.vision_tower.vision_model.encoder.layers.0.self_attn.q_proj.weight")
    import pickle

    assert pickle.loads(pickle.dumps(f)) == f


def test_no_lora_variant_freezes_nothing():
    f = Pi0Config().get_freeze_filter()
    model = _meta_model("gemma_2b", "gemma_300m")
    assert not any(f(n) for n, _ in model.named_parameters(remove_duplicate=False))
    assert not any("lora" in n for n in model.state_dict())


def test_plan_partition_of_the_frozen_model_holds_only_trainable_bytes():
    from kai0_amd.sharded import plan_partition
    from kai0_amd.train import apply_freeze_filter

    cfg = Pi0Config(paligemma_variant="gemma_2b_lora", action_expert_variant="gemma_300m_lora")
    model = _meta_model("gemma_2b_lora", "gemma_300m_lora")
    full = _meta_model("gemma_2b", "gemma_300m")
    frozen = apply_freeze_filter(model, cfg.get_freeze_filter())
    adapters = _adapter_elements(get_config("gemma_2b_lora")) + _adapter_elements(get_config("gemma_300m_lora"))
    assert sum(p.numel() for n, p in model.named_parameters() if ".lora_" in n) == adapters
    trainable = [p for p in model.parameters() if p.requires_grad]
    # trained = the adapters + everything of the plain model outside the two Gemma towers
    outside = sum(p.numel() for n, p in full.named_parameters() if not cfg.get_freeze_filter()(n))
    assert sum(p.numel() for p in trainable) == adapters + outside
    assert frozen == sum(p.numel() for n, p in full.named_parameters() if cfg.get_freeze_filter()(n))
    W = 8
    plan = plan_partition(model.sharding_units(), world_size=W, bucket_bytes=512 << 20)
    names = [u for g in plan["groups"] for u in g["units"]]
    assert [n for n in names if n.startswith("joint.")] == [f"joint.{i}" for i in range(18)]  # every layer unit still holds its adapters
    n_params = sum(b["n_params"] for g in plan["groups"] for b in g["buckets"])
    assert n_params == len(trainable)
    exact = sum(p.numel() * p.element_size() for p in trainable)
    # each parameter starts on a 256-element block and each flat buffer is a whole number of blocks per rank: at most one block of
    # padding per parameter plus W blocks per buffer
    n_buf = sum(len(g["buckets"]) for g in plan["groups"])
    assert exact <= plan["total_bytes"] <= exact + 4 * 256 * (n_params + W * n_buf)
    full_plan = plan_partition(full.sharding_units(), world_size=W, bucket_bytes=512 << 20)
    assert plan["total_bytes"] < 0.2 * full_plan["total_bytes"]  # the Gemma towers (2.9 B of 3.6 B parameters) are not in it


def _tiny_lora_model(pi05=True, dtype="float32"):
    from kai0_amd.model import PI0Pytorch

    pcfg, _ = tiny_cfgs()
    import dataclasses

    pcfg = dataclasses.replace(pcfg, paligemma_variant="dummy_lora", action_expert_variant="dummy_lora", pi05=pi05, dtype=dtype,
                               max_token_len=24)  # fmt: skip
    torch.manual_seed(5)
    model = PI0Pytorch(pcfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".lora_" in n:
                p.mul_(8.0)  # well above the 0.01 initialisation: a wrong axis or scale is far outside the tolerances
    return model, pcfg


def test_convert_round_trip_and_einsum_equations():
    model, pcfg = _tiny_lora_model()
    sd = model.state_dict()
    jp = convert.torch_to_jax(sd, siglip_heads=pcfg.siglip.num_heads)
    L, N, K, D, H, F, r = 4, 8, 1, 64, 16, 128, 8
    want = {"attn/q_einsum{}/lora_a": (L, N, D, r), "attn/q_einsum{}/lora_b": (L, N, r, H), "attn/kv_einsum{}/lora_a": (L, 2, K, D, r),
            "attn/kv_einsum{}/lora_b": (L, 2, K, r, H), "attn/attn_vec_einsum{}/lora_a": (L, N, H, r), "attn/attn_vec_einsum{}/lora_b": (L, N, r, D),
            "mlp{}/gating_einsum_lora_a": (L, 2, D, r), "mlp{}/gating_einsum_lora_b": (L, 2, r, F), "mlp{}/linear_lora_a": (L, F, r),
            "mlp{}/linear_lora_b": (L, r, D)}  # fmt: skip
    for sfx in ("", "_1"):
        for k, shp in want.items():
            assert jp[LLM + "layers/" + k.format(sfx)].shape == shp, k
    back = convert.jax_to_torch(jp, fill_missing=True)
    assert set(back) == set(sd)
    for k, v in sd.items():
        if not k.endswith("gemma_expert.lm_head.weight"):
            assert torch.equal(back[k], v), k

    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, D, generator=g).numpy()
    enc = torch.randn(2, 5, N, H, generator=g).numpy()
    act = torch.randn(2, 5, F, generator=g).numpy()
    s_attn = get_config("dummy_lora").lora_configs["attn"].scaling_value
    assert s_attn == 2.0
    pe = model.paligemma_with_expert
    for sfx, tower in (("", pe.paligemma.model.language_model), ("_1", pe.gemma_expert.model)):
        for i in (0, 3):
            at, ml = tower.layers[i].self_attn, tower.layers[i].mlp
            J = lambda name: jp[f"{LLM}layers/{name.format(sfx)}"][i]  # noqa: E731

            def dense(mod):  # the torch layout's adapter as the dense [out, in] matrix it stands for
                return lora.adapter_delta(mod.lora_a.weight.detach(), mod.lora_b.weight.detach(), *mod.lora, dtype=torch.float64).numpy()

            # lora.py:59-63 with the equations of :67-85 — q: "BTD,NDL->BTNL", "BTNL,NLH->BTNH"; the result is scaled
            q = np.einsum("BTNL,NLH->BTNH", np.einsum("BTD,NDL->BTNL", x, J("attn/q_einsum{}/lora_a")), J("attn/q_einsum{}/lora_b")) * s_attn
            assert np.allclose(q.reshape(2, 5, N * H), x @ dense(at.q_proj).T, atol=1e-5)
            kv = np.einsum("CBSKL,CKLH->CBSKH", np.einsum("BSD,CKDL->CBSKL", x, J("attn/kv_einsum{}/lora_a")), J("attn/kv_einsum{}/lora_b")) * s_attn
            assert np.allclose(kv[0].reshape(2, 5, K * H), x @ dense(at.k_proj).T, atol=1e-5)
            assert np.allclose(kv[1].reshape(2, 5, K * H), x @ dense(at.v_proj).T, atol=1e-5)
            o = np.einsum("BTNL,NLD->BTD", np.einsum("BTNH,NHL->BTNL", enc, J("attn/attn_vec_einsum{}/lora_a")), J("attn/attn_vec_einsum{}/lora_b")) * s_attn
            assert np.allclose(o, enc.reshape(2, 5, N * H) @ dense(at.o_proj).T, atol=1e-5)
            # lora.py:148: dot(dot(x, a), b), NO scaling_value (alpha = 16 would give 2)
            ga, gb = J("mlp{}/gating_einsum_lora_a"), J("mlp{}/gating_einsum_lora_b")
            assert np.allclose((x @ ga[0]) @ gb[0], x @ dense(ml.gate_proj).T, atol=1e-5)
            assert np.allclose((x @ ga[1]) @ gb[1], x @ dense(ml.up_proj).T, atol=1e-5)
            assert np.allclose((act @ J("mlp{}/linear_lora_a")) @ J("mlp{}/linear_lora_b"), act @ dense(ml.down_proj).T, atol=1e-5)
            assert ml.gate_proj.lora[0] == 1.0 and at.q_proj.lora[0] == 2.0


def test_merge_lora_against_a_float64_dense_construction():
    model, pcfg = _tiny_lora_model(dtype="bfloat16")
    sd = model.state_dict()
    merged = lora.merge_lora(sd, pcfg)
    plain, _ = tiny_cfgs()
    from kai0_amd.model import PI0Pytorch

    assert set(merged) == set(PI0Pytorch(plain).state_dict())
    N, H, r, s = 8, 16, 8, 2.0
    changed = 0
    for k, w in sd.items():
        if ".lora_" in k:
            continue
        if k[: -len("weight")] + "lora_a.weight" not in sd:
            assert merged[k] is w or torch.equal(merged[k], w), k
            continue
        a, b = sd[k[: -len("weight")] + "lora_a.weight"].double(), sd[k[: -len("weight")] + "lora_b.weight"].double()
        leaf = k.split(".")[-2]
        if leaf == "q_proj":  # per head on the output: rows n H .. of W see lora_a rows n r ..
            delta = s * torch.cat([b[n * H : (n + 1) * H] @ a[n * r : (n + 1) * r] for n in range(N)], dim=0)
        elif leaf == "o_proj":  # per head on the input: columns n H .. of W see lora_b columns n r ..
            delta = s * torch.cat([b[:, n * r : (n + 1) * r] @ a[n * r : (n + 1) * r] for n in range(N)], dim=1)
        elif leaf in ("k_proj", "v_proj"):
            delta = s * (b @ a)
        else:
            delta = b @ a  # MLP: no scale
        want = w.double() + delta
        assert merged[k].dtype == torch.bfloat16
        # W + dW formed in f32, rounded once: half a bf16 ulp of the result plus the f32 evaluation
        err = (merged[k].double() - want).abs()
        assert bool((err <= 2.0**-8 * want.abs() + 1e-6).all()), k
        assert not torch.equal(merged[k], w), k
        changed += 1
    assert changed == 2 * 4 * 7


def test_base_checkpoint_loads_into_a_lora_model(tmp_path):
    from kai0_amd.checkpoint import load_model_safetensors, save_model_safetensors
    from kai0_amd.model import PI0Pytorch

    plain_cfg, _ = tiny_cfgs()
    torch.manual_seed(1)
    base = PI0Pytorch(plain_cfg)
    path = str(tmp_path / "model.safetensors")
    save_model_safetensors(base, path)
    model, _ = _tiny_lora_model(dtype="bfloat16")
    before = {n: p.detach().clone() for n, p in model.named_parameters() if ".lora_" in n}
    load_model_safetensors(model, path)  # missing `.lora_` names are forgiven (weight_loaders.py:53-54)
    sd = model.state_dict()
    for k, v in base.state_dict().items():
        assert torch.equal(sd[k], v), k
    for n, p in model.named_parameters():
        if ".lora_" in n:
            assert torch.equal(p, before[n])
    from safetensors.torch import load_file, save_file

    part = load_file(path)
    part.pop(PWE + "gemma_expert.model.layers.1.mlp.up_proj.weight")
    short = str(tmp_path / "short.safetensors")
    save_file(part, short)
    with pytest.raises(RuntimeError, match="up_proj.weight"):
        load_model_safetensors(model, short)
    with pytest.raises(RuntimeError):  # and a LoRA checkpoint does not load into a plain model
        lp = str(tmp_path / "lora.safetensors")
        save_model_safetensors(model, lp)
        load_model_safetensors(base, lp)


def test_names_of_models_without_adapters_are_unchanged():
    """The plain tiny pi0.5 model still carries exactly the oracle's — the reference module tree's — state-dict names and shapes,
    and neither it nor the pi0 model holds adapter state anywhere."""
    import dataclasses

    from kai0_amd.model import PI0Pytorch
    from oracle.pi0_oracle import OraclePI0

    pcfg, ocfg = tiny_cfgs()
    model, oracle = PI0Pytorch(pcfg), OraclePI0(ocfg)
    got, want = model.state_dict(), oracle.state_dict()
    assert set(got) == set(want)
    assert all(got[k].shape == want[k].shape for k in want)
    for cfg in (pcfg, dataclasses.replace(pcfg, pi05=False, max_token_len=24)):
        model = PI0Pytorch(cfg)
        assert all(getattr(m, "lora", None) is None for m in model.modules()) and not any("lora" in n for n in model.state_dict())


def test_registry_entries():
    from kai0_amd.training_config import get_config as train_config

    for name, pi05 in (("debug_lora", False), ("debug_pi05_lora", True)):
        c = train_config(name)
        assert c.model.pi05 == pi05 and c.model.paligemma_variant == c.model.action_expert_variant == "dummy_lora"
        assert c.ema_decay is None and c.freeze_filter == c.model.get_freeze_filter()
        assert c.trainable_filter("x.q_proj.lora_a.weight") and not c.trainable_filter(PWE + "gemma_expert.model.norm.dense.weight")
    c = train_config("pi05_flatten_fold_lora")
    n = train_config("pi05_flatten_fold_normal")
    assert (c.model.paligemma_variant, c.model.action_expert_variant) == ("gemma_2b_lora", "gemma_300m_lora") and c.ema_decay is None
    assert c.freeze_filter == c.model.get_freeze_filter() and c.data == n.data and c.batch_size == n.batch_size
    assert n.freeze_filter is None and n.trainable_filter("anything")
