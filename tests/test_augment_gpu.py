"""csrc/augment.hip (ops.augment_images) and the per-sample augmentation through preprocess_observation and the model, on the GPU.

Reference of every parity case: `preprocessing.augment_apply_torch` on the CPU in float64.  The bound comes from the reference side only:
e_ref = max |f32 - f64| of that same function on the CPU, on the case's own inputs, and the kernel passes if
    max |kernel - f64| <= 4 e_ref + 4 * 2^-23
(4 f32 ulps at the output's magnitude of 1 as the floor; the factor 4 for a different but equally rounded f32 evaluation of the sampling
coordinates — linspace, scale, the rotated grid).  Inputs are uniform noise in [-1, 1], the worst case for interpolation error."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 28, 28), (2, 20, 36), (2, 30, 30), (5, 17, 23), (2, 224, 224)]
DEV = "cuda:0"
# forced parameter rows: crop offsets at 0 and at their maximum (-1 = maximum), the angle at -5 and at 4.999 (the corners sample outside
# and zeros come in) and at the gate (0.05), contrast and saturation at both ends
FORCED = [dict(sh=0, sw=-1, angle=-5.0, contrast=0.6, saturation=0.5), dict(sh=-1, sw=0, angle=4.999, contrast=1.4, saturation=1.5),
          dict(sh=-1, sw=-1, angle=0.05, contrast=1.4, saturation=0.5), dict(sh=0, sw=0, angle=-5.0, contrast=0.6, saturation=1.5)]  # fmt: skip


def _params(batch, height, width, geometric, variant, seed):
    """variant 0: drawn; 1, 2: the forced rows, cycled so that the gated row shares a batch with rotated ones."""
    from kai0_amd.preprocessing import sample_augment_params

    p = sample_augment_params(batch, height, width, geometric=geometric, generator=torch.Generator().manual_seed(seed))
    if variant:
        for b in range(batch):
            row = FORCED[(b + 2 * (variant - 1)) % 4]
            for name, value in row.items():
                if name in p:
                    top = {"sh": height - int(height * 0.95), "sw": width - int(width * 0.95)}.get(name)
                    p[name][b] = top if value == -1 and top is not None else value
    return p


def _reference(image, params, geometric):
    """(f64 reference [B, 3, H, W], e_ref) of an NHWC f32 CPU image."""
    from kai0_amd.preprocessing import augment_apply_torch

    ref = augment_apply_torch(image.double(), params, geometric=geometric)
    e_ref = float((augment_apply_torch(image, params, geometric=geometric).double() - ref).abs().max())
    return ref.permute(0, 3, 1, 2).contiguous(), e_ref


@functools.lru_cache(maxsize=None)
def _case(shape, geometric, variant, near_one=False):
    """One parity case, computed once and shared: (image NCHW on the device, packed rows on the device, reference f64, e_ref)."""
    from kai0_amd.preprocessing import pack_augment_params

    batch, height, width = shape
    g = torch.Generator().manual_seed(height * 1000 + width + 7 * variant)
    image = torch.rand(batch, height, width, 3, generator=g)
    image = 0.9 + 0.1 * image if near_one else image * 2 - 1
    params = _params(batch, height, width, geometric, variant, seed=batch + height)
    if near_one:
        params["brightness"][:] = 1.3
    ref, e_ref = _reference(image, params, geometric)
    rows = pack_augment_params(params, geometric=geometric).to(DEV)
    return image.permute(0, 3, 1, 2).contiguous().to(DEV), rows, ref, e_ref


def _check(got, ref, e_ref, what):
    err = float((got.double().cpu() - ref).abs().max())
    bound = 4 * e_ref + 4 * 2.0**-23
    print(f"{what}: e_ref {e_ref:.3e}  kernel {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("geometric", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_f64_definition(shape, geometric):
    from kai0_amd import ops

    for variant in (0, 1, 2):
        image, rows, ref, e_ref = _case(shape, geometric, variant)
        got = ops.augment_images(image, rows, geometric=geometric)
        assert got.shape == image.shape and got.dtype == torch.float32 and got.is_contiguous()
        _check(got, ref, e_ref, f"{shape} geometric={geometric} variant {variant}")


@pytest.mark.parametrize("geometric", [True, False])
def test_parity_where_the_clamp_saturates(geometric):
    from kai0_amd import ops

    image, rows, ref, e_ref = _case((3, 28, 28), geometric, 1, near_one=True)
    assert float((ref == 1.0).double().mean()) > 0.25  # the case does saturate
    _check(ops.augment_images(image, rows, geometric=geometric), ref, e_ref, f"near +1, brightness 1.3, geometric={geometric}")


@pytest.mark.parametrize("geometric", [True, False])
def test_batch_independence(geometric):
    from kai0_amd import ops

    image, rows, _, _ = _case((3, 28, 28), geometric, 1)
    full = ops.augment_images(image, rows, geometric=geometric)
    for b in range(3):
        one = ops.augment_images(image[b : b + 1].contiguous(), rows[b : b + 1].contiguous(), geometric=geometric)
        assert torch.equal(one[0], full[b]), b


@pytest.mark.parametrize("geometric", [True, False])
@pytest.mark.parametrize("guard", [4, 1])  # 16-byte aligned `out` (16-byte accesses), and 4-byte aligned only (scalar ones)
@pytest.mark.parametrize("shape", [(3, 28, 28), (5, 17, 23)])
def test_determinism_and_hygiene(shape, guard, geometric):
    from kai0_amd import _lib, ops

    batch, height, width = shape
    image, rows, ref, e_ref = _case(shape, geometric, 1)
    before = image.clone()
    n = image.numel()
    need = int(_lib.load().kai0_augment_scratch_floats(batch, 3, height, width))
    outs = []
    for _ in range(2):
        buf = torch.full((n + 2 * guard,), 1234.5, device=DEV)
        out = buf[guard : guard + n].view_as(image)
        out.fill_(float("nan"))
        scratch = torch.full((need + 8,), float("nan"), device=DEV)
        assert ops.augment_images(image, rows, geometric=geometric, out=out, scratch=scratch[:need]) is out
        assert not torch.isnan(out).any()
        assert bool((buf[:guard] == 1234.5).all()) and bool((buf[guard + n :] == 1234.5).all())
        assert bool(torch.isnan(scratch[need:]).all()) and not torch.isnan(scratch[:need]).any()
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(image, before)
    _check(outs[0], ref, e_ref, f"{shape} geometric={geometric} guard {guard}")
    # the access width does not change a bit: a fresh (aligned) output, and an input that is 4-byte aligned only
    assert torch.equal(outs[0], ops.augment_images(image, rows, geometric=geometric))
    shifted = torch.empty(n + 1, device=DEV)[1:].view_as(image).copy_(image)
    assert shifted.data_ptr() % 16 == 4 and torch.equal(outs[0], ops.augment_images(shifted, rows, geometric=geometric))


def test_gate_on_the_device():
    from kai0_amd import ops
    from kai0_amd.preprocessing import pack_augment_params

    image = _case((3, 28, 28), True, 0)[0]
    base = _params(3, 28, 28, True, 0, seed=31)

    def run(*angles):
        p = {**base, "angle": torch.tensor(angles, dtype=torch.float32)}
        return ops.augment_images(image, pack_augment_params(p, geometric=True).to(DEV), geometric=True)

    a, b = run(0.05, 3.0, 0.05), run(0.0, 3.0, 0.2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])


def test_refusals():
    from kai0_amd import ops
    from kai0_amd._lib import Kai0HipError

    image, rows, _, _ = _case((3, 28, 28), True, 0)
    out = torch.full_like(image, 7.0)
    with pytest.raises(Kai0HipError):
        ops.augment_images(image.double(), rows, geometric=True)
    with pytest.raises(Kai0HipError):
        ops.augment_images(image.permute(0, 1, 3, 2), rows, geometric=True)
    with pytest.raises(Kai0HipError):
        ops.augment_images(image.cpu(), rows, geometric=True)
    with pytest.raises(Kai0HipError, match="overlap"):
        ops.augment_images(image, rows, geometric=True, out=image)
    with pytest.raises(Kai0HipError, match="overlap"):  # a shifted view of the same buffer
        both = torch.zeros(2 * image.numel(), device=DEV)
        half = image.numel() // 2
        ops.augment_images(both[: image.numel()].view_as(image), rows, geometric=True, out=both[half : half + image.numel()].view_as(image))
    four = torch.zeros(3, 4, 28, 28, device=DEV)
    with pytest.raises(Kai0HipError, match="C=4"):
        ops.augment_images(four, rows, geometric=True, out=torch.full_like(four, 7.0))
    low = torch.zeros(3, 3, 4, 28, device=DEV)
    low_out = torch.full_like(low, 7.0)
    with pytest.raises(Kai0HipError, match="H=4"):
        ops.augment_images(low, rows, geometric=True, out=low_out)
    with pytest.raises(Kai0HipError):
        ops.augment_images(image, rows[:2].contiguous(), geometric=True, out=out)
    assert bool((out == 7.0).all()) and bool((low_out == 7.0).all())  # nothing was launched


def test_through_the_model():
    from tiny import build_pair, obs_to

    from kai0_amd.preprocessing import IMAGE_KEYS, _augment, sample_augment_params
    from oracle.pi0_oracle import synthetic_batch

    dev = torch.device(DEV)
    model, _, _, ocfg = build_pair(dev, seed=0, std=0.08)
    obs, actions, noise, time = synthetic_batch(ocfg, 2, seed=0)
    gobs = obs_to(obs, dev)
    seed = 77
    # the images the trunk gets, against the definition with the parameters the same seed draws on the CPU
    torch.manual_seed(seed)
    images = model._preprocess_observation(gobs, train="per_sample")[0]
    torch.manual_seed(seed)
    for key, got in zip(IMAGE_KEYS, images):
        geometric = "wrist" not in key
        params = sample_augment_params(2, 56, 56, geometric=geometric)
        ref, e_ref = _reference(obs.images[key].permute(0, 2, 3, 1).contiguous(), params, geometric)
        assert got.shape == obs.images[key].shape
        _check(got, ref, e_ref, f"model {key}")
    assert not torch.equal(images[0][0] - gobs.images[IMAGE_KEYS[0]][0], images[0][1] - gobs.images[IMAGE_KEYS[0]][1])
    # forward: finite, and the same seed gives the same bits
    model.train_augmentation = "per_sample"
    losses = []
    for _ in range(2):
        torch.manual_seed(seed)
        with torch.no_grad():
            losses.append(model(gobs, actions.to(dev), noise=noise.to(dev), time=time.to(dev)))
    assert bool(torch.isfinite(losses[0]).all()) and torch.equal(losses[0], losses[1])
    torch.manual_seed(seed + 1)
    with torch.no_grad():
        assert not torch.equal(model(gobs, actions.to(dev), noise=noise.to(dev), time=time.to(dev)), losses[0])
    # True is still the per-batch form: _augment under the same seed on the device, bit for bit
    model.train_augmentation = True
    torch.manual_seed(seed)
    images = model._preprocess_observation(gobs, train=model.train_augmentation)[0]
    torch.manual_seed(seed)
    for key, got in zip(IMAGE_KEYS, images):
        want = _augment(gobs.images[key].permute(0, 2, 3, 1), geometric="wrist" not in key).permute(0, 3, 1, 2)
        assert torch.equal(got, want), key
