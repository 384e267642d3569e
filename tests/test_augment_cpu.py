"""Per-sample train augmentation, host side (kai0_amd/preprocessing.py: sample_augment_params, augment_apply_torch, the `augment`
keyword of preprocess_observation; KAI0_AUGMENT in train.build_model; the C ABI of csrc/augment.hip).

The new definition is tied to the existing one: with the same six values for every sample `augment_apply_torch` must give
`_augment`'s bits, and `_augment` is pinned to the reference's own code by test_preprocessing_reference_cpu.py."""

import ctypes as C
import os
import re
import types

import pytest
import torch

from kai0_amd import preprocessing as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("base_0_rgb", "left_wrist_0_rgb", "right_wrist_0_rgb")


def _image(batch, height, width, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(batch, height, width, 3, generator=g) * 2 - 1


def _replay_scalar_draws(batch, height, width, geometric):
    """`_augment`'s draws from the default generator, in its order, every sample given the same values."""
    p = {}
    if geometric:
        p["sh"] = torch.full((batch,), int(torch.randint(0, height - int(height * 0.95) + 1, (1,), device="cpu")))
        p["sw"] = torch.full((batch,), int(torch.randint(0, width - int(width * 0.95) + 1, (1,), device="cpu")))
        p["angle"] = torch.full((batch,), float(torch.rand(1) * 10 - 5))
    p["brightness"] = torch.full((batch,), 0.7 + float(torch.rand(1)) * 0.6, dtype=torch.float64)
    p["contrast"] = torch.full((batch,), 0.6 + float(torch.rand(1)) * 0.8, dtype=torch.float64)
    p["saturation"] = torch.full((batch,), 0.5 + float(torch.rand(1)) * 1.0, dtype=torch.float64)
    return p


@pytest.mark.parametrize("geometric", [True, False])
@pytest.mark.parametrize("shape", [(3, 28, 28), (2, 20, 36), (2, 30, 30)])
def test_restatement_gives_the_existing_paths_bits(shape, geometric):
    image = _image(*shape)
    for seed in (0, 1, 2, 3):  # several draws: angles on both sides of the gate, crop offsets 0 and > 0
        torch.manual_seed(seed)
        want = P._augment(image, geometric)
        torch.manual_seed(seed)
        params = _replay_scalar_draws(*shape, geometric)
        got = P.augment_apply_torch(image, params, geometric=geometric)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(got, want), (seed, float((got - want).abs().max()))


def test_sample_augment_params_ranges_dtypes_and_generators():
    B, H, W = 64, 28, 36
    torch.manual_seed(5)
    p = P.sample_augment_params(B, H, W, geometric=True)
    assert list(p) == ["sh", "sw", "angle", "brightness", "contrast", "saturation"]  # the draw order
    assert all(v.shape == (B,) and v.device.type == "cpu" for v in p.values())
    assert p["sh"].dtype == torch.int64 and p["sw"].dtype == torch.int64
    assert all(p[k].dtype == torch.float32 for k in ("angle", "brightness", "contrast", "saturation"))
    assert 0 <= int(p["sh"].min()) and int(p["sh"].max()) <= H - int(0.95 * H)
    assert 0 <= int(p["sw"].min()) and int(p["sw"].max()) <= W - int(0.95 * W)
    for key, lo, hi in (("angle", -5.0, 5.0), ("brightness", 0.7, 1.3), ("contrast", 0.6, 1.4), ("saturation", 0.5, 1.5)):
        assert float(p[key].min()) >= lo and float(p[key].max()) < hi + 1e-6, key
        assert float(p[key].max() - p[key].min()) > 0.5 * (hi - lo), key  # 64 draws cover the range
    # the vectorised draws in the documented order, formed as _augment forms its scalars
    torch.manual_seed(5)
    assert torch.equal(p["sh"], torch.randint(0, H - int(H * 0.95) + 1, (B,)))
    assert torch.equal(p["sw"], torch.randint(0, W - int(W * 0.95) + 1, (B,)))
    assert torch.equal(p["angle"], torch.rand(B) * 10 - 5)
    assert torch.equal(p["brightness"], 0.7 + torch.rand(B) * 0.6)
    assert torch.equal(p["contrast"], 0.6 + torch.rand(B) * 0.8)
    assert torch.equal(p["saturation"], 0.5 + torch.rand(B) * 1.0)
    # same seed, same tensors; the default generator is consumed
    torch.manual_seed(5)
    before = torch.get_rng_state()
    q = P.sample_augment_params(B, H, W, geometric=True)
    assert all(torch.equal(p[k], q[k]) for k in p)
    assert not torch.equal(torch.get_rng_state(), before)
    # an explicit generator leaves the default one alone and reproduces itself
    before = torch.get_rng_state()
    r1 = P.sample_augment_params(B, H, W, geometric=True, generator=torch.Generator().manual_seed(9))
    r2 = P.sample_augment_params(B, H, W, geometric=True, generator=torch.Generator().manual_seed(9))
    assert torch.equal(torch.get_rng_state(), before)
    assert all(torch.equal(r1[k], r2[k]) for k in r1) and not torch.equal(r1["angle"], p["angle"])
    # colour only: three draws
    torch.manual_seed(5)
    c = P.sample_augment_params(B, H, W, geometric=False)
    assert list(c) == ["brightness", "contrast", "saturation"]
    torch.manual_seed(5)
    assert torch.equal(c["brightness"], 0.7 + torch.rand(B) * 0.6)
    # per sample: a batch of 8 does not share one angle
    torch.manual_seed(0)
    assert P.sample_augment_params(8, H, W, geometric=True)["angle"].unique().numel() > 1


def test_rotation_gate_is_decided_per_sample():
    image = _image(3, 28, 28)
    torch.manual_seed(0)
    p = P.sample_augment_params(3, 28, 28, geometric=True)

    def with_angles(*angles):
        return P.augment_apply_torch(image, {**p, "angle": torch.tensor(angles, dtype=torch.float32)}, geometric=True)

    a, b = with_angles(0.05, 3.0, 0.05), with_angles(0.0, 3.0, 0.2)
    assert torch.equal(a[0], b[0])  # 0.05 is below the gate: not resampled a second time
    assert torch.equal(a[1], b[1])
    assert not torch.equal(a[2], b[2])  # 0.2 is rotated
    assert torch.equal(with_angles(-0.05, 3.0, 0.0)[0], b[0])


def _obs(images):
    batch = next(iter(images.values())).shape[0]
    return types.SimpleNamespace(images=images, image_masks={}, state=torch.zeros(batch, 32), tokenized_prompt=None, tokenized_prompt_mask=None)


@pytest.mark.parametrize("channels_first", [True, False])
def test_default_form_is_untouched(channels_first):
    nhwc = {k: _image(2, 28, 28, seed=i) for i, k in enumerate(KEYS)}
    images = nhwc
    if channels_first:  # _augment sees the NHWC view of the NCHW tensor: same values, another memory order under its reductions
        images = {k: v.permute(0, 3, 1, 2).contiguous() for k, v in nhwc.items()}
        nhwc = {k: v.permute(0, 2, 3, 1) for k, v in images.items()}
    torch.manual_seed(11)
    want = {k: P._augment(nhwc[k], geometric="wrist" not in k) for k in KEYS}
    state = torch.get_rng_state()
    for kw in ({}, {"augment": "batch"}):
        torch.manual_seed(11)
        got = P.preprocess_observation(_obs(images), train=True, **kw)
        assert torch.equal(torch.get_rng_state(), state), kw
        for k in KEYS:
            g = got.images[k].permute(0, 2, 3, 1) if channels_first else got.images[k]
            assert torch.equal(g, want[k]), (kw, k)
    # no augmentation, no draw
    torch.manual_seed(11)
    state = torch.get_rng_state()
    got = P.preprocess_observation(_obs(images), train=False, augment="per_sample")
    assert torch.equal(torch.get_rng_state(), state)
    assert all(torch.equal(got.images[k], images[k]) for k in KEYS)
    with pytest.raises(ValueError, match="per_sample"):
        P.preprocess_observation(_obs(images), train=True, augment="sample")


@pytest.mark.parametrize("channels_first", [True, False])
def test_per_sample_form_on_cpu_tensors(channels_first):
    B, H, W = 3, 20, 36
    nhwc = {k: _image(B, H, W, seed=i) for i, k in enumerate(KEYS)}
    images = nhwc
    if channels_first:
        images = {k: v.permute(0, 3, 1, 2).contiguous() for k, v in nhwc.items()}
        nhwc = {k: v.permute(0, 2, 3, 1) for k, v in images.items()}
    torch.manual_seed(21)
    got = P.preprocess_observation(_obs(images), train=True, augment="per_sample")
    state = torch.get_rng_state()
    torch.manual_seed(21)  # the cameras draw in image_keys order
    params = {k: P.sample_augment_params(B, H, W, geometric="wrist" not in k) for k in KEYS}
    assert torch.equal(torch.get_rng_state(), state)
    for k in KEYS:
        g = got.images[k]
        assert g.shape == images[k].shape
        g = g.permute(0, 2, 3, 1) if channels_first else g
        for b in range(B):
            one = {name: v[b : b + 1] for name, v in params[k].items()}
            assert torch.equal(g[b : b + 1], P.augment_apply_torch(nhwc[k][b : b + 1], one, geometric="wrist" not in k)), (k, b)
    assert params["base_0_rgb"]["angle"].unique().numel() == B  # the samples really differ


def test_pack_augment_params_rows():
    import numpy as np

    p = {"sh": torch.tensor([0, 2]), "sw": torch.tensor([1, 0]), "angle": torch.tensor([0.05, -5.0]),
         "brightness": torch.tensor([0.7, 1.3]), "contrast": torch.tensor([0.6, 1.4]), "saturation": torch.tensor([0.5, 1.5])}  # fmt: skip
    rows = P.pack_augment_params(p, geometric=True)
    assert rows.dtype == torch.float32 and rows.shape == (2, 8)
    rad = -5.0 * torch.pi / 180.0
    want = torch.tensor([[0, 1, np.cos(0.05 * torch.pi / 180), np.sin(float(np.float32(0.05)) * torch.pi / 180), 0, 0.7, 0.6, 0.5],
                         [2, 0, np.cos(rad), np.sin(rad), 1, 1.3, 1.4, 1.5]], dtype=torch.float32)  # fmt: skip
    assert torch.allclose(rows, want, rtol=0, atol=1e-9)
    colour = P.pack_augment_params({k: p[k] for k in ("brightness", "contrast", "saturation")}, geometric=False)
    assert torch.equal(colour[:, :5], torch.zeros(2, 5)) and torch.equal(colour[:, 5:], rows[:, 5:])


def test_header_binding_and_abi():
    from kai0_amd import _lib
    from kai0_amd.build import SRC

    header = open(os.path.join(ROOT, "include", "kai0hip.h")).read()
    assert re.search(r"int kai0_augment_f32\(const float\* in, float\* out, const float\* params, float\* scratch,\s*int B, int C, int H, "
                     r"int W, int geometric,\s*kai0_stream_t stream\);", header)  # fmt: skip
    assert re.search(r"int64_t kai0_augment_scratch_floats\(int B, int C, int H, int W\);", header)
    doc = header[header.index("Train-time image augmentation") : header.index("int kai0_augment_f32(")]
    assert "preprocessing_pytorch.py:52-142" in doc
    p, i = C.c_void_p, C.c_int
    assert _lib._PROTOS["kai0_augment_f32"] == [p, p, p, p, i, i, i, i, i, p]
    assert {"kai0_augment_f32", "kai0_augment_scratch_floats"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "augment.hip" in SRC and _lib.ABI_VERSION == 4
    lib = _lib.load()
    assert lib.kai0_abi_version() == 4
    # the scratch size needs no device: one float per block of 1024 pixels and sample; 0 outside the contract
    assert lib.kai0_augment_scratch_floats(32, 3, 224, 224) == 32 * 49
    assert lib.kai0_augment_scratch_floats(3, 3, 17, 23) == 3
    assert lib.kai0_augment_scratch_floats(3, 4, 28, 28) == 0 and lib.kai0_augment_scratch_floats(3, 3, 4, 28) == 0
    # refusals come before any launch, so they need no device either
    buf = (C.c_float * 4096)()
    a = C.addressof(buf)
    for args, word in (((a, a + 8192, a + 4096, a + 4224, 1, 4, 8, 8, 1), "C=4"), ((a, a + 8192, a + 4096, a + 4224, 1, 3, 4, 8, 1), "H=4"),
                       ((a, a + 256, a + 4096, a + 4224, 1, 3, 8, 8, 1), "overlap")):  # fmt: skip
        assert lib.kai0_augment_f32(*args, None) != 0
        assert word in lib.kai0_last_error().decode(), lib.kai0_last_error()


def test_augment_images_has_no_cpu_form():
    from kai0_amd import ops
    from kai0_amd._lib import Kai0HipError

    with pytest.raises(Kai0HipError):
        ops.augment_images(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8), geometric=True)


def test_KAI0_AUGMENT_parsing(monkeypatch):
    import dataclasses

    from kai0_amd import train

    monkeypatch.delenv("KAI0_AUGMENT", raising=False)
    assert train.augment_mode_from_env() == "batch"
    for value in ("batch", "per_sample"):
        monkeypatch.setenv("KAI0_AUGMENT", value)
        assert train.augment_mode_from_env() == value
    for value in ("1", "sample", "", "PER_SAMPLE"):
        monkeypatch.setenv("KAI0_AUGMENT", value)
        with pytest.raises(ValueError, match="'batch' or 'per_sample'"):
            train.augment_mode_from_env()

    # build_model: the switch sets the model's train_augmentation, and nothing when it is unset or `batch`
    class Model(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.train_augmentation = True

    @dataclasses.dataclass
    class ModelConfig:
        dtype: str = "bfloat16"

        def _model_class(self):
            return Model

    config = types.SimpleNamespace(model=ModelConfig(), pytorch_training_precision="bfloat16", pytorch_weight_path=None,
                                   advantage_estimator=False)  # fmt: skip
    for value, want in ((None, True), ("batch", True), ("per_sample", "per_sample")):
        monkeypatch.delenv("KAI0_AUGMENT", raising=False)
        if value is not None:
            monkeypatch.setenv("KAI0_AUGMENT", value)
        assert train.build_model(config, "cpu").train_augmentation == want and (want is True) == (value != "per_sample")
    monkeypatch.setenv("KAI0_AUGMENT", "sample")
    with pytest.raises(ValueError, match="'batch' or 'per_sample'"):
        train.build_model(config, "cpu")


def test_model_refuses_an_unknown_train_augmentation():
    from kai0_amd.model import PI0Pytorch

    with pytest.raises(ValueError, match="per_sample"):
        PI0Pytorch._preprocess_observation(None, None, train="persample")
