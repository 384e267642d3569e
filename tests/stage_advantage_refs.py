"""Restatements for Stage-Advantage annotation (kai0_amd/stage_advantage.py, csrc/frames.hip).  A plain helper module like
tests/streaming_refs.py: nothing here touches the HIP library, everything runs on the CPU.

One restatement per operation, written after its description in include/kai0hip.h:
  * `frames_to_chw_ref`   — kai0_frames_to_chw in numpy f32, operation for operation (the fused multiply-adds of the source index and of
                            the tap accumulation are the kernel's explicit fmaf calls; nothing else fuses: numpy never does, and
                            the library is built with -ffp-contract=off).  tests/test_stage_advantage_cpu.py calibrates it against
                            `kai0_amd.preprocessing.resize_with_pad_torch` on the evaluator's normalised input; the GPU is then held to it.
  * `prefix_gather_ref`   — kai0_prefix_gather as torch indexing + cat (a copy: bit-exact).
  * `stub_values`         — the stand-in for `model.sample_values` of the executed-reference golden (make_stage_advantage_golden.py):
                            a fixed seeded projection of the images an observation carries, through tanh.  No model: the golden pins
                            WHICH frames reach the model in which slot, and the evaluator's post-processing."""

import numpy as np
import torch

F32 = np.float32


def resize_geometry(h0, w0, height, width):
    """resize_with_pad_torch's own arithmetic (shared/image_tools.py:88-113), Python floats."""
    ratio = max(w0 / width, h0 / height)
    rh, rw = int(h0 / ratio), int(w0 / ratio)
    return rh, rw, (height - rh) // 2, (width - rw) // 2


def _fma(a, b, c):
    """fmaf(a, b, c) on f32 arrays: the product of two f32 values is exact in f64, the sum rounds once to f64 and once to f32 (the
    second rounding can differ from a true fused operation's in rare ties: one f32 ulp, inside the GPU test's 1e-6)."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def _taps(size_in, size_out):
    """torch's align_corners=False source index in f32: (i0, i1, lambda) per output index.  src = fma(scale, dst + 0.5, -0.5): torch's
    CPU build contracts `scale * (dst + 0.5) - 0.5` (area_pixel_compute_source_index) into one fused operation, and with src up to
    H0 an unfused product moves lambda by up to an ulp of H0."""
    scale = F32(size_in) / F32(size_out)
    dst = np.arange(size_out, dtype=F32)
    src = np.maximum(_fma(scale, dst + F32(0.5), F32(-0.5)), F32(0.0)).astype(F32)
    i0 = np.minimum(src.astype(np.int32), size_in - 1)
    i1 = np.minimum(i0 + 1, size_in - 1)
    lam = (src - i0.astype(F32)).astype(F32)
    return i0, i1, lam


def frames_to_chw_ref(frames: np.ndarray, height: int, width: int) -> np.ndarray:
    """uint8 [N, H0, W0, 3] -> f32 [N, 3, height, width] (kai0hip.h kai0_frames_to_chw)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    n, h0, w0, _ = frames.shape
    rh, rw, ph0, pw0 = resize_geometry(h0, w0, height, width)
    v = (frames.astype(F32) / F32(255.0) * F32(2.0) - F32(1.0)).astype(F32)  # [N, H0, W0, 3]
    y0, y1, ly = _taps(h0, rh)
    x0, x1, lx = _taps(w0, rw)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    wy0, wx0 = F32(1.0) - ly, F32(1.0) - lx
    v00, v01, v10, v11 = v[:, y0][:, :, x0], v[:, y0][:, :, x1], v[:, y1][:, :, x0], v[:, y1][:, :, x1]
    acc = ((wy0 * lx).astype(F32) * v01).astype(F32)  # the four tap weights are products of the axis weights, rounded to f32 ...
    acc = _fma((wy0 * wx0).astype(F32), v00, acc)  # ... and the taps are accumulated in this order, one fused multiply-add each
    acc = _fma((ly * wx0).astype(F32), v10, acc)
    acc = _fma((ly * lx).astype(F32), v11, acc)
    inner = np.clip(acc, F32(-1.0), F32(1.0)).astype(F32)  # [N, rh, rw, 3]
    out = np.full((n, 3, height, width), F32(-1.0), dtype=F32)
    out[:, :, ph0 : ph0 + rh, pw0 : pw0 + rw] = inner.transpose(0, 3, 1, 2)
    return out


def evaluator_image(frame: np.ndarray, height: int, width: int) -> torch.Tensor:
    """The evaluator's `_process_single_image` (evaluator.py:151-165) with the project's resize_with_pad_torch -> f32 [3, H, W]."""
    from kai0_amd.preprocessing import resize_with_pad_torch

    t = torch.from_numpy(np.ascontiguousarray(frame)).float() / 255.0
    t = t * 2.0 - 1.0
    return resize_with_pad_torch(t, height, width)[0].permute(2, 0, 1).contiguous()


def prefix_gather_ref(bank: torch.Tensor, slots, lang: torch.Tensor | None) -> torch.Tensor:
    """bank [cap, n_img, D], slots [B][nslot], lang None | [T, D] | [B, T, D] -> [B, nslot * n_img + T, D]."""
    idx = torch.as_tensor(slots, dtype=torch.int64, device=bank.device)
    B, nslot = idx.shape
    parts = [bank[idx].reshape(B, nslot * bank.shape[1], bank.shape[2])]
    if lang is not None:
        parts.append(lang if lang.dim() == 3 else lang[None].expand(B, -1, -1))
    return torch.cat(parts, dim=1)


# ---- the golden's stand-in model -------------------------------------------------------------------------------------------------
STUB_SEED = 20251019
_ORDER = {"base": 0, "left_wrist": 1, "right_wrist": 2}


def stub_weights(n_images: int, size: int = 224) -> np.ndarray:
    """f64 [n_images, 3, size, size], scaled so that the projection of images uniform in [-1, 1] has unit variance."""
    w = np.random.default_rng(STUB_SEED + n_images).standard_normal((n_images, 3, size, size))
    return w / (np.sqrt(n_images * 3 * size * size / 3.0))


def stub_values_from_stack(images: np.ndarray) -> np.ndarray:
    """images [B, n_images, 3, S, S] in (timestep, camera) order -> f32 [B]: tanh of the f64 projection, rounded to f32 once."""
    w = stub_weights(images.shape[1], images.shape[-1])
    z = np.einsum("bnchw,nchw->b", np.asarray(images, dtype=np.float64), w)
    return np.tanh(z).astype(F32)


def stub_sample_values(device, observation) -> torch.Tensor:
    """`model.sample_values(device, observation)` of the golden: images sorted as preprocess_observation_custom sorts them."""

    def key(k):
        part, ts, _ = k.rsplit("_", 2)
        return int(ts), _ORDER[part]

    keys = sorted(observation.images, key=key)
    stack = np.stack([observation.images[k].detach().cpu().numpy() for k in keys], axis=1)
    return torch.from_numpy(stub_values_from_stack(stack))[:, None]
