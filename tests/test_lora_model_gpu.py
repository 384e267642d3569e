"""The LoRA model end to end on the GPU: the tiny model with "dummy_lora" on both towers (pi0.5, and one pi0 case) and one case at
the real widths, against the UNMODIFIED fp32 oracle loaded with the merged weights W + dW formed in float64 from the same bf16
values (an adapter is, mathematically, that dense weight):
  * loss tensor rel-L2 < 1e-2;
  * adapter gradients through the chain rule from the oracle's dW (dA = s B^T dW, dB = s dW A^T, per head where grouped) and
    every trainable non-adapter gradient, rel-L2 <= 5e-2; mathematically zero / absent gradients as in
    tests/test_model_gpu.py::test_backward_matches_oracle_autograd;
  * the frozen set = get_freeze_filter(); frozen parameters get no .grad, no optimizer state and keep their bits over three
    Trainer.train_step calls while the loss falls;
  * sample_actions equals, bit for bit, that of a plain model loaded from merge_lora(...), and stays within the chunk bounds of
    the fp32 oracle on the merged weights (rel-L2 < 1e-2, max < 2e-2); a train step after a chunk drops the engine;
  * train_loop("debug_pi05_lora") resumes exactly.
(The bounds are the ones tests/test_model_gpu.py holds the plain model to against the fp32 oracle and the reference-executed backward.)"""

import copy
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


# ------------------------------------------------------------------ the dense weight an adapter stands for, and its chain rule
def _spec(name, cfg):
    """(scale, heads_up, heads_down) of the adapted Linear `name` (…q_proj etc.), from the layout table of kai0_amd/lora.py."""
    leaf = name.rsplit(".", 1)[-1]
    if leaf in ("gate_proj", "up_proj", "down_proj"):
        return 1.0, 1, 1  # FeedForward._dot: no scale
    s = cfg.lora_configs["attn"].scaling_value
    return {"q_proj": (s, cfg.num_heads, 1), "k_proj": (s, 1, 1), "v_proj": (s, 1, 1), "o_proj": (s, 1, cfg.num_heads)}[leaf]


def _delta(a, b, s, hu, hd):
    a, b = a.to(F64), b.to(F64)
    if hu > 1:  # rows n H .. of W see lora_a rows n r ..
        r, H = b.shape[1], b.shape[0] // hu
        return s * torch.cat([b[n * H : (n + 1) * H] @ a[n * r : (n + 1) * r] for n in range(hu)], dim=0)
    if hd > 1:  # columns n H .. of W see lora_b columns n r ..
        r = a.shape[0] // hd
        return s * torch.cat([b[:, n * r : (n + 1) * r] @ a[n * r : (n + 1) * r] for n in range(hd)], dim=1)
    return s * (b @ a)


def _chain(dW, a, b, s, hu, hd):
    """(dA, dB) from dW of the merged weight."""
    dW, a, b = dW.to(F64), a.to(F64), b.to(F64)
    if hu > 1:
        r, H = b.shape[1], b.shape[0] // hu
        dA = torch.cat([b[n * H : (n + 1) * H].T @ dW[n * H : (n + 1) * H] for n in range(hu)], dim=0)
        dB = torch.cat([dW[n * H : (n + 1) * H] @ a[n * r : (n + 1) * r].T for n in range(hu)], dim=0)
    elif hd > 1:
        r, H = a.shape[0] // hd, a.shape[1]
        dA = torch.cat([b[:, n * r : (n + 1) * r].T @ dW[:, n * H : (n + 1) * H] for n in range(hd)], dim=0)
        dB = torch.cat([dW[:, n * H : (n + 1) * H] @ a[n * r : (n + 1) * r].T for n in range(hd)], dim=1)
    else:
        dA, dB = b.T @ dW, dW @ a.T
    return s * dA, s * dB


def _tower_cfg(name, model):
    pe = model.paligemma_with_expert
    return pe.exp_cfg if ".gemma_expert." in name else pe.vlm_cfg


def _adapted(model):
    """[(prefix of the Linear, a, b, spec)] over the model's state dict."""
    sd = model.state_dict()
    out = []
    for k in sd:
        if k.endswith(".lora_a.weight"):
            pre = k[: -len(".lora_a.weight")]
            out.append((pre, sd[pre + ".lora_a.weight"], sd[pre + ".lora_b.weight"], _spec(pre, _tower_cfg(pre, model))))
    return out


def _merged_f64(model):
    """The plain variant's state dict with W + dW in float64 (other tensors as they are)."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if ".lora_" not in k}
    for pre, a, b, spec in _adapted(model):
        sd[pre + ".weight"] = sd[pre + ".weight"].to(F64) + _delta(a.cpu(), b.cpu(), *spec)
    return sd


def _seed_adapters(model, std=0.04, seed=7):
    """Adapters large enough that dW is a sizeable share of W (std 0.08 here): the 0.01 initialisation would hide a wrong adapter
    behind the base weight's rounding."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".lora_" in n:
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.dtype))


def _build(pi05=True):
    """(LoRA HIP model on the GPU, fp32 reference on the merged weights, batch)."""
    from tiny import obs_to, tiny_cfgs

    from kai0_amd.model import PI0Pytorch
    from oracle.pi0_oracle import OraclePI0, synthetic_batch, synthetic_weights_

    pcfg, ocfg = tiny_cfgs()
    if pi05:
        base = OraclePI0(ocfg)
        synthetic_weights_(base, seed=0)
        with torch.no_grad():
            for _, p in base.named_parameters():
                if p.dim() >= 2:
                    p.mul_(0.08 / 0.02)
        ref = OraclePI0(ocfg)
    else:
        import pi0_restatement as R

        ocfg = R.pi0_cfg(ocfg)
        probe = R.RestatedPI0(ocfg)
        base = R.build_restated(dataclasses.replace(ocfg, pi05=True), R.seeded_pi0_only(probe, seed=11, std=0.08), 0.08)
        ref = R.RestatedPI0(ocfg)
    lcfg = dataclasses.replace(pcfg, paligemma_variant="dummy_lora", action_expert_variant="dummy_lora", pi05=pi05,
                               discrete_state_input=None, max_token_len=pcfg.max_token_len)  # fmt: skip
    torch.manual_seed(3)
    model = PI0Pytorch(lcfg)
    missing, unexpected = model.load_state_dict(base.state_dict(), strict=False)
    assert not unexpected and all(".lora_" in k for k in missing)
    _seed_adapters(model)
    model.train_augmentation = False
    model = model.to(DEV)
    ref.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    ref.load_state_dict({k: v.to(torch.float32) for k, v in _merged_f64(model).items()}, strict=True)
    obs, actions, noise, time = synthetic_batch(ocfg, 2, seed=0)
    return dict(model=model, ref=ref.eval(), cfg=lcfg, obs=obs, gobs=obs_to(obs, DEV), actions=actions, noise=noise, time=time)


@pytest.fixture(scope="module")
def lp():
    return _build(True)


def _freeze(case):
    from kai0_amd.train import apply_freeze_filter

    f = case["cfg"].get_freeze_filter()
    apply_freeze_filter(case["model"], f)
    return f


def _check_loss_and_grads(case, what, n_adapters, grad_tol=5e-2):
    """`n_adapters`: how many adapter matrices must have been compared — all of them but the ones of the Linears without a consumer, the
    last prefix layer's q_proj (its queries feed prefix rows nobody reads), o_proj and MLP: 2 x (7 x depth - 5) + 2 x 7 x depth."""
    m, ref = case["model"], case["ref"]
    f = _freeze(case)
    m.zero_grad(set_to_none=True)
    loss = m(case["gobs"], case["actions"].to(DEV), noise=case["noise"].to(DEV), time=case["time"].to(DEV))
    loss.mean().backward()
    ref.zero_grad(set_to_none=True)
    ref_loss = ref(case["obs"], case["actions"], case["noise"], case["time"])
    ref_loss.mean().backward()
    r = rel(loss.detach(), ref_loss.detach())
    print(f"{what}: loss rel-L2 vs the fp32 oracle on merged weights {r:.3e}")
    assert loss.shape == ref_loss.shape and r < 1e-2
    gm = {n: p.grad for n, p in m.named_parameters()}
    go = {n: p.grad for n, p in ref.named_parameters()}
    want = {}
    for pre, a, b, spec in _adapted(m):
        dW = go[pre + ".weight"]
        want[pre + ".lora_a.weight"], want[pre + ".lora_b.weight"] = (None, None) if dW is None else _chain(dW, a.cpu(), b.cpu(), *spec)
    for n, g in go.items():
        if f(n):
            assert gm[n] is None, f"{n} is frozen and must not receive a gradient"
        else:
            want[n] = g
    assert set(want) == {n for n, p in m.named_parameters() if p.requires_grad}
    table, bad = [], []
    for n, g in want.items():
        if g is None:  # no consumer: the last prefix layer's o_proj / MLP (nothing reads the prefix after the last joint attention)
            assert gm[n] is None or float(gm[n].abs().max()) == 0.0, f"{n} must not receive a gradient"
            continue
        assert gm[n] is not None, f"no gradient for {n}"
        if float(g.norm()) < 1e-8:  # mathematically zero (SigLIP key bias: softmax is shift-invariant)
            assert float(gm[n].float().norm()) < 1e-4, n
            continue
        e = rel(gm[n], g)
        table.append((e, n))
        if e > grad_tol:
            bad.append((e, n))
    table.sort(reverse=True)
    for e, n in table[:5]:
        print(f"  {e:.3e}  {n}")
    n_ad = sum(".lora_" in n for _, n in table)
    print(f"{what}: checked {len(table)} gradients ({n_ad} adapters), worst rel-L2 {table[0][0]:.3e} ({table[0][1]})")
    assert not bad, f"{len(bad)} gradient mismatches, worst: {sorted(bad, reverse=True)[:5]}"
    assert n_ad == n_adapters and len(table) - n_ad >= 30  # (30: SigLIP, projector and heads of the smallest case)
    m.zero_grad(set_to_none=True)


def test_loss_and_gradients_match_the_oracle_on_merged_weights(lp):
    _check_loss_and_grads(lp, "pi05", n_adapters=2 * (7 * 4 - 5) + 2 * 7 * 4)


def test_pi0_loss_and_gradients_match_the_restatement_on_merged_weights():
    _check_loss_and_grads(_build(False), "pi0", n_adapters=2 * (7 * 4 - 5) + 2 * 7 * 4)


def test_gradient_checkpointing_gives_the_same_gradients(lp):
    m = lp["model"]
    _freeze(lp)
    args = (lp["gobs"], lp["actions"].to(DEV))
    kw = dict(noise=lp["noise"].to(DEV), time=lp["time"].to(DEV))
    m.train()
    m.zero_grad(set_to_none=True)
    m(*args, **kw).mean().backward()
    plain = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    m.gradient_checkpointing_enable()
    try:
        m(*args, **kw).mean().backward()
    finally:
        m.gradient_checkpointing_disable()
    for n, g in plain.items():
        got = dict(m.named_parameters())[n].grad
        assert got is not None and rel(got, g) < 1e-2, n  # the expert's chain runs on one stream under remat: same values, other order
    m.zero_grad(set_to_none=True)


def test_frozen_set_and_three_train_steps(lp):
    from kai0_amd.train import Trainer

    case = _build(True)
    m = case["model"]
    f = _freeze(case)
    names = dict(m.named_parameters(remove_duplicate=False))
    assert {n for n, p in names.items() if not p.requires_grad} == {n for n in names if f(n)}
    assert all(p.requires_grad for n, p in names.items() if ".lora_" in n)
    frozen_before = {n: p.detach().clone() for n, p in names.items() if f(n)}
    adapters_before = {n: p.detach().clone() for n, p in names.items() if ".lora_" in n}
    m.train()
    tr = Trainer(m, peak_lr=2e-3, warmup_steps=1, decay_steps=10, end_lr=2e-4)
    losses = [float(tr.train_step(case["gobs"], case["actions"].to(DEV), case["noise"].to(DEV), case["time"].to(DEV))) for _ in range(4)]
    print("losses", losses)
    assert losses[-1] < losses[0]
    for n, p in names.items():
        if f(n):
            assert p.grad is None and torch.equal(p.detach(), frozen_before[n]), n
    moved = sum(not torch.equal(p.detach(), adapters_before[n]) for n, p in names.items() if ".lora_" in n)
    assert moved >= 0.9 * len(adapters_before)  # (the last prefix layer's o_proj / MLP adapters have no consumer)
    sd = tr.engine.state_dict(tr._param_order)
    with_state = {sd["param_names"][i] for i in sd["state"]}
    dead = "paligemma_with_expert.gemma_expert.lm_head.weight"
    assert with_state == {n for n, p in m.named_parameters() if p.requires_grad and n != dead}
    assert not any(f(n) for n in with_state)


def test_chunk_equals_the_merged_plain_model_and_the_oracle(lp):
    from tiny import tiny_cfgs

    from kai0_amd import lora
    from kai0_amd.model import PI0Pytorch
    from kai0_amd.train import Trainer

    m, ref = lp["model"], lp["ref"]
    m.eval()
    noise = lp["noise"].to(DEV)
    out = m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10)
    assert torch.equal(out, m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10))
    plain_cfg, _ = tiny_cfgs()
    plain = PI0Pytorch(plain_cfg)
    plain.load_state_dict(lora.merge_lora(m.state_dict(), lp["cfg"]), strict=True)
    plain.train_augmentation = False
    plain = plain.to(DEV).eval()
    want = plain.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10)
    assert torch.equal(out, want), f"LoRA model's chunk differs from the merged plain model's: rel-L2 {rel(out, want):.3e}"
    with torch.no_grad():
        ref_out = ref.sample_actions(lp["obs"], lp["noise"], num_steps=10)
    r, mx = rel(out, ref_out), float((out.cpu() - ref_out).abs().max())
    print(f"LoRA chunk vs the fp32 oracle on merged weights: rel-L2 {r:.3e}, max|d| {mx:.3e}")
    assert r < 1e-2 and mx < 2e-2
    # ... and the merge is no no-op: the chunk of the base weights alone is another one
    base = PI0Pytorch(plain_cfg)
    base.load_state_dict({k: v for k, v in m.state_dict().items() if ".lora_" not in k}, strict=True)
    base.train_augmentation = False
    assert not torch.equal(base.to(DEV).eval().sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10), out)
    # an in-place edit of an adapter behind autograd is noticed by the content stamp, like an edit of a base weight
    eng = m._engine
    torch.cuda.synchronize()
    assert eng is not None and not m.inference_is_stale()
    a = m.paligemma_with_expert.gemma_expert.model.layers[0].self_attn.q_proj.lora_a.weight
    saved = a.data.clone()
    a.data.mul_(3.0)
    m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10)
    torch.cuda.synchronize()
    assert m.inference_is_stale()
    edited = m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10)
    assert m._engine is not eng and not torch.equal(edited, out)
    a.data.copy_(saved)
    m.invalidate_inference_engine()
    assert torch.equal(m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10), out)
    # a train step after a chunk invalidates the engine
    _freeze(lp)
    m.train()
    m.eval()
    m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10)
    assert m._engine is not None
    keep = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr = Trainer(m, peak_lr=1e-3, warmup_steps=1, decay_steps=10, end_lr=1e-4)
    m.train()
    tr.train_step(lp["gobs"], lp["actions"].to(DEV), lp["noise"].to(DEV), lp["time"].to(DEV))
    assert m._engine is None
    m.eval()
    after = m.sample_actions(DEV, lp["gobs"], noise=noise, num_steps=10)
    assert not torch.equal(after, out)
    m.set_unit_hooks(None)
    with torch.no_grad():  # leave the shared fixture as it was
        for n, p in m.named_parameters():
            p.copy_(keep[n])
    m.invalidate_inference_engine()


@pytest.mark.timeout(600)
def test_train_loop_debug_pi05_lora_resume_is_exact(tmp_path):
    """`train_loop(get_config("debug_pi05_lora"))`: 6 steps in one go against the same run stopped after 4 and resumed to 6 — the
    optimizer state holds the trainable parameters only (indexed by position in model.parameters(), no entry for frozen ones), and
    steps 4 and 5 log the same loss, learning rate and gradient norm."""
    import dataclasses as dc

    from kai0_amd import training_config as tc
    from kai0_amd.train import train_loop

    base = dc.replace(tc.get_config("debug_pi05_lora"), checkpoint_base_dir=str(tmp_path / "ckpt"), assets_base_dir=str(tmp_path / "assets"),
                      num_workers=0, num_train_steps=6, log_interval=1, save_interval=100,
                      lr_schedule=tc.CosineDecaySchedule(warmup_steps=2, peak_lr=1e-3, decay_steps=10, decay_lr=1e-4))  # fmt: skip
    full = train_loop(dc.replace(base, exp_name="full", overwrite=True))
    assert [r["step"] for r in full] == list(range(6)) and all(r["loss"] == r["loss"] for r in full)
    ck = tmp_path / "ckpt" / "debug_pi05_lora" / "full" / "6"
    assert sorted(os.listdir(ck)) == ["metadata.pt", "model.safetensors", "optimizer.pt"]
    opt = torch.load(ck / "optimizer.pt", weights_only=False)
    f = base.freeze_filter
    names = opt["param_names"]
    assert any(".lora_a." in n for n in names) and any(f(n) for n in names)  # every parameter has a position ...
    assert not any(f(names[i]) for i in opt["state"]) and any(".lora_b." in names[i] for i in opt["state"])  # ... state only the trained
    part = train_loop(dc.replace(base, exp_name="cut", num_train_steps=4, overwrite=True))
    assert [r["loss"] for r in part] == [r["loss"] for r in full[:4]]
    rest = train_loop(dc.replace(base, exp_name="cut", overwrite=False, resume=True))
    assert [r["step"] for r in rest] == [4, 5]
    for a, b in zip(rest, full[4:]):
        assert a["loss"] == b["loss"] and a["grad_norm"] == b["grad_norm"] and a["learning_rate"] == b["learning_rate"], (a, b)
    print("debug_pi05_lora loss curve", [round(r["loss"], 5) for r in full], "resumed", [round(r["loss"], 5) for r in rest])


def test_real_widths_loss_and_adapter_gradients():
    """Gemma-2B / 300M widths (2048 / 1024, head_dim 256, mlp 16384 / 4096), ranks 16 / 32, depth 1, one SigLIP layer, B = 1, a
    16-token prompt: every adapter product in the kernel configuration of the real model (kai0_lora_down at R = 32 / 64 / 16,
    kai0_lora_wgrad, the batched per-head GEMMs at H = 256), against the fp32 oracle on the merged weights."""
    from fullwidth import _depth
    from tiny import obs_to

    from kai0_amd.config import Pi0Config, SiglipConfig
    from kai0_amd.model import PI0Pytorch
    from oracle import pi0_oracle as O

    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    with _depth(1):
        ocfg = O.OracleConfig(dtype="bfloat16", vocab_size=2048, max_token_len=16, siglip=O.SiglipCfg(num_layers=1))
        base, ref = O.OraclePI0(ocfg), O.OraclePI0(ocfg)
        O.synthetic_weights_(base, seed=0)
        lcfg = Pi0Config(paligemma_variant="gemma_2b_lora", action_expert_variant="gemma_300m_lora", vocab_size=2048, max_token_len=16,
                         siglip=SiglipConfig(num_layers=1))  # fmt: skip
        torch.manual_seed(3)
        model = PI0Pytorch(lcfg)
    pe = model.paligemma_with_expert
    assert (pe.vlm_cfg.width, pe.vlm_cfg.mlp_dim, pe.vlm_cfg.head_dim, pe.vlm_cfg.lora_configs["attn"].rank) == (2048, 16384, 256, 16)
    assert (pe.exp_cfg.width, pe.exp_cfg.mlp_dim, pe.exp_cfg.lora_configs["ffn"].rank) == (1024, 4096, 32)
    missing, unexpected = model.load_state_dict(base.state_dict(), strict=False)
    assert not unexpected and all(".lora_" in k for k in missing)
    _seed_adapters(model, std=0.01)  # W is N(0, 0.02) here: dW = B A at rank 16 .. 32 is then ~10 % of W
    model.train_augmentation = False
    model = model.to(DEV)
    ref.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    ref.load_state_dict({k: v.to(torch.float32) for k, v in _merged_f64(model).items()}, strict=True)
    obs, actions, noise, time = O.synthetic_batch(ocfg, 1, seed=3)
    case = dict(model=model, ref=ref.eval(), cfg=lcfg, obs=obs, gobs=obs_to(obs, DEV), actions=actions, noise=noise, time=time)
    _check_loss_and_grads(case, "real_widths", n_adapters=2 * (7 * 1 - 5) + 2 * 7 * 1)
