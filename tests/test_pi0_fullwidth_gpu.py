"""pi0 (`pi05=False`) at the real widths, depth 2 (tests/fullwidth.py's method): Gemma-2B + 300M expert joint layers, SigLIP so400m
layers, three 224^2 cameras, pi0's 48 prompt slots, 1 state token + 50 action tokens — P = 816, 51 suffix rows, S = 867 — against the
CPU restatement (tests/pi0_restatement.py, pinned to the reference-executed fixture by tests/test_pi0_cpu.py), at the bounds
tests/test_fullwidth_gpu.py holds pi0.5 to: loss rel-L2 <= 1e-2 (bf16 and fp32 restatement); chunk rel-L2 <= 3e-3 and max|d| <= 2e-2
vs the bf16 restatement, rel-L2 <= 1e-2 vs the fp32 one."""

import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

F32 = torch.float32
N_JOINT, N_SIG = 2, 2


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def dev():
    return torch.device("cuda:0")


def build_pi0_restated(n_joint=N_JOINT, n_sig=N_SIG, seed=0):
    """the pi0 builder next to fullwidth.build_oracle: the oracle's synthetic weights, the expert's plain norm weights N(0, 0.1)
    instead of 0 so that the (1 + w) factor (and its fold into the projection weights) is exercised"""
    import pi0_restatement as R
    from fullwidth import _depth

    from oracle import pi0_oracle as O

    with _depth(n_joint):
        cfg = O.OracleConfig(vocab_size=2048, pi05=False, max_token_len=48, siglip=O.SiglipCfg(num_layers=n_sig))
        m = R.RestatedPI0(cfg)
    O.synthetic_weights_(m, seed=seed)
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".gemma_expert.model." in k and k.endswith("norm.weight"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return m.eval(), cfg


def build_pi0_hip(restated, n_joint=N_JOINT, n_sig=N_SIG):
    from fullwidth import _depth

    from kai0_amd.config import Pi0Config, SiglipConfig
    from kai0_amd.model import PI0Pytorch

    with _depth(n_joint):
        model = PI0Pytorch(Pi0Config(pi05=False, vocab_size=2048, siglip=SiglipConfig(num_layers=n_sig)))
    model.load_state_dict(restated.state_dict(), strict=True)
    model.train_augmentation = False
    return model.to(dev())


@pytest.fixture(scope="module")
def fw():
    from tiny import obs_to

    from oracle.pi0_oracle import synthetic_batch

    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    restated, cfg = build_pi0_restated()
    model = build_pi0_hip(restated)
    obs, actions, noise, time = synthetic_batch(cfg, 2, seed=3)
    r32 = copy.deepcopy(restated)
    r32.paligemma_with_expert.to_bfloat16_for_selected_params("float32")
    return dict(model=model, ref=restated, ref32=r32, obs=obs, gobs=obs_to(obs, dev()), actions=actions, noise=noise, time=time)


def test_pi0_fullwidth_loss_matches_restatement(fw):
    m, d = fw["model"], dev()
    assert fw["obs"].tokenized_prompt.shape == (2, 48) and not bool(fw["obs"].tokenized_prompt_mask.all())
    with torch.no_grad():
        loss = m(fw["gobs"], fw["actions"].to(d), noise=fw["noise"].to(d), time=fw["time"].to(d))
        ref = fw["ref"](fw["obs"], fw["actions"], fw["noise"], fw["time"])
        ref32 = fw["ref32"](fw["obs"], fw["actions"], fw["noise"], fw["time"])
    r, r32 = rel(loss, ref), rel(loss, ref32)
    print(f"pi0 full-width loss: rel-L2 {r:.3e} vs bf16 restatement, {r32:.3e} vs fp32 (bf16 vs fp32 restatement {rel(ref, ref32):.3e})")
    assert loss.shape == (2, 50, 32) and loss.dtype == F32
    assert r <= 1e-2 and r32 <= 1e-2


@pytest.mark.parametrize("batch", [2, 1])
def test_pi0_fullwidth_chunk_matches_restatement_on_the_production_stack(fw, batch):
    from test_fullsize_gpu import _take

    from kai0_amd.infer import InferenceEngine

    m, d = fw["model"], dev()
    m.eval()
    try:
        gobs, obs, noise = fw["gobs"], fw["obs"], fw["noise"]
        if batch == 1:
            gobs, obs, noise = _take(gobs, 1), _take(obs, 1), noise[1:2]
        m.invalidate_inference_engine()
        out = m.sample_actions(d, gobs, noise=noise.to(d), num_steps=10)
        eng = m._engine
        assert eng.fast and (eng.P, eng.Ss, eng.S) == (816, 51, 867)
        with torch.no_grad():
            ref = fw["ref"].sample_actions(obs, noise, num_steps=10)
            ref32 = fw["ref32"].sample_actions(obs, noise, num_steps=10)
        r, r32, mx = rel(out, ref), rel(out, ref32), float((out.cpu() - ref).abs().max())
        print(f"pi0 full-width chunk B={batch}: rel-L2 {r:.3e} (max|d| {mx:.3e}) vs bf16 restatement, {r32:.3e} vs fp32")
        assert out.shape == (batch, 50, 32) and out.dtype == F32
        assert r <= 3e-3 and mx <= 2e-2 and r32 <= 1e-2
        assert torch.equal(out, m.sample_actions(d, gobs, noise=noise.to(d), num_steps=10))  # replay is deterministic
        InferenceEngine.force_generic = True
        try:
            m.invalidate_inference_engine()
            generic = m.sample_actions(d, gobs, noise=noise.to(d), num_steps=10)
            assert not m._engine.fast
        finally:
            InferenceEngine.force_generic = False
        print(f"pi0 chunk B={batch}: production (folded) stack vs generic per-layer path rel-L2 {rel(out, generic):.3e}")
        assert rel(out, generic) <= 3e-3
    finally:
        m.invalidate_inference_engine()
        m.train()
