"""pi0 (`pi05=False`) without a GPU: the CPU restatement pinned to the reference-executed fixture, the HIP model's parameter tree
against the reference's state-dict contract, the sharding partition and the JAX <-> torch key map."""

import json
import os
import sys

import numpy as np
import pytest
import torch
from safetensors import safe_open
from safetensors.torch import load_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
FIX = os.path.join(HERE, "golden", "reference_pi0.safetensors")


@pytest.fixture(scope="module")
def fixture():
    with safe_open(FIX, "pt") as f:
        meta = json.loads(f.metadata()["json"])
    return load_file(FIX), meta


@pytest.fixture(scope="module")
def restated(fixture):
    import pi0_restatement as R
    from tiny import tiny_cfgs

    E, meta = fixture
    _, ocfg05 = tiny_cfgs()
    return R.build_restated(ocfg05, {k[2:]: v for k, v in E.items() if k.startswith("w.")}, float(meta["std"]))


def _tiny_pi0_config():
    import dataclasses

    from tiny import tiny_cfgs

    pcfg, _ = tiny_cfgs()
    return dataclasses.replace(pcfg, pi05=False, discrete_state_input=None)


def test_restatement_equals_reference_executed_fixture_exactly(fixture, restated):
    """loss, 10-step chunk, suffix embedding / pad / att and the listed gradients of the restatement equal what the reference's own
    code computed (make_reference_pi0_golden.py), max|d| = 0.0 — as the pi0.5 oracle does against reference_e2e."""
    from oracle.pi0_oracle import synthetic_batch

    E, _ = fixture
    obs, actions, noise, time = synthetic_batch(restated.config, 2, seed=0)
    assert torch.equal(noise, E["noise"]) and torch.equal(time, E["time"]) and torch.equal(actions, E["in_actions"])
    with torch.no_grad():
        t = time[:, None, None]
        suf, pad, att, cond = restated.embed_suffix_state(obs.state, t * noise + (1 - t) * actions, time)
        loss = restated(obs, actions, noise, time)
        chunk = restated.sample_actions(obs, noise.clone(), num_steps=10)
    assert cond is None and suf.shape == (2, 11, 64) and att[0].tolist() == [1.0, 1.0] + [0.0] * 9
    assert torch.equal(suf, E["suffix"]) and torch.equal(pad, E["suffix_pad"]) and torch.equal(att.float(), E["suffix_att"])
    assert torch.equal(loss, E["loss"]), float((loss - E["loss"]).abs().max())
    assert torch.equal(chunk, E["actions"]), float((chunk - E["actions"]).abs().max())
    restated.zero_grad(set_to_none=True)
    restated(obs, actions, noise, time).mean().backward()
    params = dict(restated.named_parameters())
    for k in [k[5:] for k in E if k.startswith("grad.")]:
        assert torch.equal(params[k].grad, E["grad." + k]), k
    restated.zero_grad(set_to_none=True)


def test_fixture_noise_floor_is_at_most_half_the_bounds(fixture):
    _, meta = fixture
    assert float(meta["floor_loss_rel_l2"]) <= 0.5e-2 and float(meta["floor_chunk_rel_l2"]) <= 1.5e-3


def test_pi0_model_constructs_with_the_reference_state_dict(fixture, restated):
    """keys, shapes and dtypes of PI0Pytorch(pi05=False) equal the reference's list; the fixture's weights load strictly."""
    from kai0_amd.model import PI0Pytorch

    _, meta = fixture
    model = PI0Pytorch(_tiny_pi0_config())
    want = meta["state_dict_keys"]
    got = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in model.state_dict().items()}
    assert got == want
    assert not any(k.startswith("time_mlp") or ".dense." in k for k in got)
    assert {"state_proj.weight", "action_time_mlp_in.weight", "action_time_mlp_out.bias",
            "paligemma_with_expert.gemma_expert.model.norm.weight"} <= set(got)  # fmt: skip
    assert got["action_time_mlp_in.weight"] == [[64, 128], "float32"]
    model.load_state_dict(restated.state_dict(), strict=True)


def test_pi0_sharding_units_partition_the_parameters():
    from kai0_amd.model import PI0Pytorch

    model = PI0Pytorch(_tiny_pi0_config())
    units = model.sharding_units()
    ids = [id(p) for _, ps in units for p in ps]
    dead = model.paligemma_with_expert.gemma_expert.lm_head.weight
    assert len(ids) == len(set(ids)), "a parameter is in two units"
    assert set(ids) == {id(p) for p in model.parameters() if p is not dead}
    prefix = {id(p) for p in dict(units)["prefix"]}
    for head in (model.state_proj, model.action_time_mlp_in, model.action_time_mlp_out, model.action_in_proj):
        assert all(id(p) in prefix for p in head.parameters())


def test_pi05_key_set_is_unchanged():
    """the pi0.5 parameter tree still is the oracle's (= the reference's, tests/test_reference_blocks_cpu.py)"""
    from tiny import tiny_cfgs

    from kai0_amd.model import PI0Pytorch
    from oracle.pi0_oracle import OraclePI0

    pcfg, ocfg = tiny_cfgs()
    got = {k: (tuple(v.shape), v.dtype) for k, v in PI0Pytorch(pcfg).state_dict().items()}
    want = {k: (tuple(v.shape), v.dtype) for k, v in OraclePI0(ocfg).state_dict().items()}
    assert got == want
    assert "time_mlp_in.weight" in got and "state_proj.weight" not in got


def test_advantage_estimator_refuses_pi0_clearly():
    from kai0_amd.model import AdvantageEstimator

    with pytest.raises(NotImplementedError, match="pi0.5 trunk only"):
        AdvantageEstimator(_tiny_pi0_config())


def test_convert_round_trip_on_a_synthetic_pi0_tree(restated):
    """torch -> JAX tree -> torch reproduces every tensor; the JAX side carries the names of models/pi0.py:97-99 and the `scale`
    parameters of the non-adaptive expert (gemma.py:119-125 with `_name(.., 1)`), and no adaRMS / pi0.5 entries."""
    from kai0_amd import convert

    sd = {k: v for k, v in restated.state_dict().items() if not k.endswith("lm_head.weight")}
    tree = convert.torch_to_jax(sd, num_heads=8, num_kv_heads=1, siglip_heads=4)
    llm = "PaliGemma/llm/"
    assert tree["state_proj/kernel"].shape == (32, 64) and tree["action_time_mlp_in/kernel"].shape == (128, 64)
    assert tree["action_time_mlp_out/kernel"].shape == (64, 64) and tree["action_time_mlp_out/bias"].shape == (64,)
    assert tree[llm + "layers/pre_attention_norm_1/scale"].shape == (4, 64) and tree[llm + "layers/pre_ffw_norm_1/scale"].shape == (4, 64)
    assert tree[llm + "final_norm_1/scale"].shape == (64,)
    assert not any(("norm" in k and "Dense_0" in k) or k.startswith("time_mlp") for k in tree)
    # axis convention of nnx.Linear: y = x @ kernel + bias
    x = torch.randn(3, 128, generator=torch.Generator().manual_seed(0))
    y = torch.nn.functional.linear(x, sd["action_time_mlp_in.weight"], sd["action_time_mlp_in.bias"])
    np.testing.assert_allclose(x.numpy() @ tree["action_time_mlp_in/kernel"] + tree["action_time_mlp_in/bias"], y.numpy(), rtol=1e-5, atol=1e-6)
    back = convert.jax_to_torch(tree, fill_missing=True, vocab_size=304)
    assert set(back) == set(restated.state_dict())
    for k, v in sd.items():
        assert torch.equal(back[k].float(), v.float()), k
    assert back["paligemma_with_expert.gemma_expert.lm_head.weight"].shape == (304, 64)
    # a pi0.5 tree still takes the adaRMS branch
    from tiny import tiny_cfgs

    from oracle.pi0_oracle import OraclePI0

    sd05 = OraclePI0(tiny_cfgs()[1]).state_dict()
    tree05 = convert.torch_to_jax(sd05, siglip_heads=4)
    assert llm + "final_norm_1/Dense_0/kernel" in tree05 and "state_proj/kernel" not in tree05
    assert "paligemma_with_expert.gemma_expert.model.norm.dense.weight" in convert.jax_to_torch(tree05)


def test_split_sum_form_of_the_suffix_mlp_is_within_one_bf16_ulp_of_the_cat_form():
    """What the inference engine's hoisting does to the arithmetic, on the CPU in f32 torch: W_in[:, :De] a + (W_in[:, De:] te + b_in)
    against the reference's single Linear over cat[a, te] — f32 sums reordered, so after the MLP's second Linear a bf16 rounding may
    flip: at most one ulp (pi0_restatement.within_one_bf16_ulp: plus the f32 level itself at the output's zero crossings), and rarely
    (measured: 99.955 % of the elements bit-equal; >= 99 % is what the GPU kernel test asks)."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(0)
    M, De = 100, 1024
    a, te = torch.randn(M, De, generator=g), torch.randn(De, generator=g)
    w_in, b_in = torch.randn(De, 2 * De, generator=g) * De**-0.5, torch.randn(De, generator=g) * 0.1
    w_out, b_out = torch.randn(De, De, generator=g) * 2 * De**-0.5, torch.randn(De, generator=g) * 0.1
    cat32 = F.linear(F.silu(F.linear(torch.cat([a, te[None].expand(M, De)], 1), w_in, b_in)), w_out, b_out)
    tvec = F.linear(te[None], w_in[:, De:], b_in)[0]
    split = F.linear(F.silu(F.linear(a, w_in[:, :De]) + tvec), w_out, b_out).to(torch.bfloat16)

    import pi0_restatement as R

    h = F.silu(F.linear(torch.cat([a, te[None].expand(M, De)], 1), w_in, b_in))
    mag = h.abs() @ w_out.abs().t() + b_out.abs()  # sum of the magnitudes of the terms of every output element
    ok, share = R.within_one_bf16_ulp(split, cat32, mag)
    far = (split.float() - cat32.to(torch.bfloat16).float()).abs() > R.bf16_ulp(cat32)
    print(f"split-sum vs cat form: {int(far.sum())} of {far.numel()} elements more than one bf16 ulp apart (all at |ref| <= "
          f"{float(cat32[far].abs().max()) if bool(far.any()) else 0.0:.2e}: zero crossings), equal share {share:.5f}")
    assert bool(ok.all()) and share >= 0.99
    assert not bool(far.any()) or float(cat32[far].abs().max()) < 1e-3  # beyond one ulp only where the result itself is ~0
