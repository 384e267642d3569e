"""Stage-Advantage step 2 on the HIP path: annotate every frame of a dataset with a trained `AdvantageEstimator`, then discretise
the annotations into `task_index` labels (stage_advantage/annotation/{evaluator,eval,discretize_advantage}.py).

    python -m kai0_amd.stage_advantage annotate   <repo_id> --config ADVANTAGE_TORCH_KAI0_FLATTEN_FOLD --ckpt <dir> --steps 100000
    python -m kai0_amd.stage_advantage discretize <data_path> --threshold 30 --discretion-type binary --stage-nums 2

The evaluator drives `sample_values` one six-image observation batch at a time: every frame's three cameras pass through SigLIP as the
"previous" and the "current" image of the relative pass and as the "current" image of the absolute pass, frame 0 is encoded again for
every batch, the ~10-token prompt is padded to 200 masked rows, and the frames become f32 on host threads.  `ValueAnnotator` keeps the
episode's working set on the device instead:

  * frames are uploaded as uint8 and prepared by `kai0_frames_to_chw` (the evaluator's `_process_single_image`);
  * every image goes through `embed_image` ONCE per episode; the features live in a ring bank of `relative_interval + batch_size`
    frames plus a fixed slot for frame 0, so memory does not grow with the episode;
  * `kai0_prefix_gather` assembles the prefixes of a whole batch (relative pass [frame n | frame min(n + D, F - 1)], absolute pass
    [frame 0 | frame n], the (-100, 0) timestep order `preprocess_observation_custom` sorts to) straight out of the bank;
  * the prompt is embedded once and cut to its valid length rounded up to 8 (known on the host: no device read), the mask codes are
    built once per episode on one row.

The joint forward and the value head are the model's own (`embed_suffix`, `forward_joint`, `AdvantageEstimator._value`), so LoRA
estimators work unchanged.  `plan_episode`, `advantages_from_values`, `annotate_dataset` and `discretize` are host code and need no GPU.
"""

from __future__ import annotations

import argparse
import dataclasses
import glob
import json
import logging
import os
import pathlib
from collections.abc import Callable, Sequence

import numpy as np

logger = logging.getLogger("kai0_amd")

CAMERA_KEYS = ("top_head", "hand_left", "hand_right")  # eval.py:170-178, in the model's (base, left_wrist, right_wrist) order
ADVANTAGE_COLUMNS = ("relative_advantage", "absolute_value", "absolute_advantage")  # eval.py:112
DEFAULT_PROMPT = "Flatten and fold the cloth."  # eval.py:200
NCAM = 3


# ------------------------------------------------------------------------------------------------ episode plan
@dataclasses.dataclass(frozen=True)
class BatchPlan:
    """One batch of an episode.  Slot tables hold FRAME slots of the ring (`ring_slot`), one row per sample; the engine expands a frame
    slot s to the image slots 3 s + camera.  `fill` = [lo, hi): the frames to encode before this batch runs (ascending, each once)."""

    frames: tuple[int, ...]
    futures: tuple[int, ...]
    fill: tuple[int, int]
    relative_slots: tuple[tuple[int, ...], ...] | None  # [frame n | frame future]; None in one-timestep mode
    absolute_slots: tuple[tuple[int, ...], ...]  # [frame 0 | frame n]; one-timestep mode: [frame n]


def ring_size(relative_interval: int, batch_size: int) -> int:
    return relative_interval + batch_size + 1


def ring_slot(frame: int, relative_interval: int, batch_size: int) -> int:
    """Frame 0 owns slot 0 for the whole episode; frame f > 0 lives at 1 + (f - 1) mod (relative_interval + batch_size).  A batch
    [s, s + B) reads frames s .. s + B - 1 + relative_interval at most: B + relative_interval <= the modulus consecutive frames, so no
    two of them share a slot, and the frame a fill overwrites lies before s."""
    return 0 if frame == 0 else 1 + (frame - 1) % (relative_interval + batch_size)


def plan_episode(num_frames: int, relative_interval: int = 50, batch_size: int = 16, two_timesteps: bool = True) -> list[BatchPlan]:
    """The evaluator's batching (evaluator.py:324-332, 549-557): batches of consecutive frames, future = min(n + interval, F - 1)."""
    if num_frames < 2:
        raise ValueError(f"Insufficient frames: {num_frames}, need at least 2")
    if relative_interval < 1 or batch_size < 1:
        raise ValueError(f"relative_interval = {relative_interval} and batch_size = {batch_size} must be positive")
    last = num_frames - 1
    slot = lambda f: ring_slot(f, relative_interval, batch_size)  # noqa: E731
    plans, filled = [], 0
    for start in range(0, num_frames, batch_size):
        frames = tuple(range(start, min(start + batch_size, num_frames)))
        futures = tuple(min(n + relative_interval, last) for n in frames)
        need = (max(futures) if two_timesteps else frames[-1]) + 1
        fill = (filled, max(filled, need))
        filled = fill[1]
        if two_timesteps:
            rel = tuple((slot(n), slot(f)) for n, f in zip(frames, futures))
            ab = tuple((slot(0), slot(n)) for n in frames)
        else:
            rel, ab = None, tuple((slot(n),) for n in frames)
        plans.append(BatchPlan(frames, futures, fill, rel, ab))
    return plans


def advantages_from_values(absolute_values, relative_values=None, *, relative_interval: int = 50) -> dict[str, np.ndarray]:
    """The evaluator's post-processing (evaluator.py:442-481, 623-650) of the f32 model outputs, in float64 as its Python floats are:
    frame 0's absolute value is 0; the relative value is 0 where the future frame is the frame itself and is rescaled by
    interval / gap where the future was clamped to the last frame; absolute_advantage = absolute_value[future] - absolute_value[n] with
    the same rescaling, from the unclamped values; both advantages are clamped to [-1, 1] last.  `relative_values=None`: the
    one-timestep mode (no `relative_advantage` in the result)."""
    av = np.asarray(absolute_values, dtype=np.float32).reshape(-1).astype(np.float64)
    n = av.shape[0]
    if n < 2:
        raise ValueError(f"Insufficient frames: {n}, need at least 2")
    frame = np.arange(n, dtype=np.int64)
    future = np.minimum(frame + relative_interval, n - 1)
    gap = future - frame
    same, full = gap == 0, gap == relative_interval
    safe = np.where(same, 1, gap).astype(np.float64)
    av[0] = 0.0
    out = {"frame_idx": frame, "future_frame_idx": future}
    if relative_values is not None:
        rv = np.asarray(relative_values, dtype=np.float32).reshape(-1).astype(np.float64)
        if rv.shape[0] != n:
            raise ValueError(f"{rv.shape[0]} relative values for {n} absolute values")
        rel = np.where(full, rv, np.where(same, 0.0, rv / safe * relative_interval))
        out["relative_advantage"] = np.clip(rel, -1.0, 1.0)
    diff = av[future] - av
    adv = np.where(full, diff, np.where(same, 0.0, diff / safe * relative_interval))
    out["absolute_value"] = av
    out["absolute_advantage"] = np.clip(adv, -1.0, 1.0)
    return out


# ------------------------------------------------------------------------------------------------ the engine
class ValueAnnotator:
    """Per-frame values of whole episodes from a resident, eval-mode `AdvantageEstimator` on one GPU (module docstring)."""

    def __init__(self, model, *, batch_size: int = 16, siglip_batch: int = 96, trim_prompt: bool = True):
        from .model import AdvantageEstimator

        if not isinstance(model, AdvantageEstimator):
            raise TypeError(f"ValueAnnotator needs an AdvantageEstimator, got {type(model).__name__}")
        if model.training:
            raise ValueError("ValueAnnotator needs the estimator in eval mode (model.eval())")
        hooks = model.paligemma_with_expert.unit_hooks
        if getattr(hooks, "mode", None) == "fsdp":
            raise ValueError("ValueAnnotator needs the parameters resident on one GPU: the model's unit hooks shard them (mode 'fsdp')")
        if batch_size < 1 or siglip_batch < NCAM:
            raise ValueError(f"batch_size = {batch_size} must be positive and siglip_batch = {siglip_batch} at least {NCAM}")
        self.model = model
        self.batch_size, self.siglip_batch, self.trim_prompt = int(batch_size), int(siglip_batch), bool(trim_prompt)
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise ValueError("ValueAnnotator: the estimator is not on a GPU; the product path has no CPU fallback")
        self.images_encoded = 0  # images through SigLIP since construction (each frame's three cameras count once per episode)
        self._ep = None

    # ---- per-episode state --------------------------------------------------------------------------------
    def _begin(self, frames, tokens, token_mask, two_timesteps: bool, relative_interval: int):
        import torch

        from . import ops
        from .model import BF16, build_mask_codes

        if len(frames) != NCAM:
            raise ValueError(f"Expected {NCAM} frame arrays (top, left, right), got {len(frames)}")
        frames = [np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f.contiguous().cpu().numpy() for f in frames]
        F = frames[0].shape[0]
        for f in frames:
            if f.dtype != np.uint8 or f.ndim != 4 or f.shape[-1] != 3:
                raise TypeError(f"frames must be uint8 [F, H0, W0, 3], got {f.dtype} {f.shape}")
            if f.shape[0] != F:
                raise ValueError(f"Inconsistent frame counts: {[g.shape[0] for g in frames]}")
        plans = plan_episode(F, relative_interval, self.batch_size, two_timesteps)
        m, pe, dev = self.model, self.model.paligemma_with_expert, self.device
        wait = getattr(pe.unit_hooks, "wait_params", None)
        if wait is not None:  # a sharded (zero2) trainer owns the parameters: its in-flight all-gathers must have landed
            wait()
        res = pe.siglip_cfg.image_size
        n_img = pe.paligemma.model.vision_tower.vision_model.embeddings.num_patches
        D = pe.siglip_cfg.projection_dim
        tokens = np.asarray(tokens).reshape(-1)
        mask = np.asarray(token_mask).astype(bool).reshape(-1)
        if tokens.shape != mask.shape:
            raise ValueError(f"tokens {tokens.shape} and token_mask {mask.shape} differ")
        keep = T = tokens.shape[0]
        if self.trim_prompt:  # PI0Pytorch._trim_prompt with the length taken on the host
            last = int(np.flatnonzero(mask)[-1]) + 1 if mask.any() else 0
            keep = min(T, max(8, (last + 7) // 8 * 8))
        table = pe.paligemma.model.language_model.embed_tokens.weight
        lang = ops.embed(table, torch.from_numpy(tokens[None, :keep].astype(np.int64)).to(dev), ops.sqrt_scale(D)).view(keep, D)
        nslot = 2 * NCAM if two_timesteps else NCAM
        Hs = m.config.action_horizon
        pad = torch.cat([torch.ones(nslot * n_img, dtype=torch.bool), torch.from_numpy(mask[:keep]), torch.ones(Hs, dtype=torch.bool)])
        att = torch.zeros(pad.shape[0], dtype=torch.bool)
        att[nslot * n_img + keep] = True  # embed_suffix (pi0.5): the first action token opens the suffix block
        codes = build_mask_codes(pad[None].to(dev), att[None].to(dev))
        ring = ring_size(relative_interval, self.batch_size)
        bank = torch.empty((ring * NCAM, n_img, D), dtype=BF16, device=dev)
        self._ep = dict(frames=frames, F=F, plans=plans, res=res, n_img=n_img, D=D, lang=lang, keep=keep, nslot=nslot, Hs=Hs, codes=codes,
                        bank=bank, filled=0, interval=relative_interval, two=two_timesteps, batch_codes={})  # fmt: skip
        return self._ep

    def _fill(self, lo: int, hi: int) -> None:
        """Encode frames [lo, hi) (ascending, each exactly once per episode) into their ring slots."""
        import torch

        from . import ops

        ep = self._ep
        if lo != ep["filled"] or hi < lo:
            raise RuntimeError(f"ring fill out of order: frames [{lo}, {hi}) after {ep['filled']} filled")
        pe, per = self.model.paligemma_with_expert, max(1, self.siglip_batch // NCAM)
        n_img, D, bank = ep["n_img"], ep["D"], ep["bank"]
        for g0 in range(lo, hi, per):
            g1 = min(g0 + per, hi)
            host = np.stack([f[g0:g1] for f in ep["frames"]], axis=1)  # [n, cam, H0, W0, 3]: images in (frame, camera) order
            u8 = torch.from_numpy(host.reshape(-1, *host.shape[2:])).to(self.device)  # uint8 over the bus, a plain synchronous copy
            feats = pe.embed_image(ops.frames_to_chw(u8, ep["res"], ep["res"]))  # [n * cam, n_img, D]
            self.images_encoded += feats.shape[0]
            g = g0
            while g < g1:  # runs of consecutive ring slots (a run ends where the ring wraps, and after frame 0's fixed slot)
                s0 = ring_slot(g, ep["interval"], self.batch_size)
                run = 1
                while g + run < g1 and ring_slot(g + run, ep["interval"], self.batch_size) == s0 + run:
                    run += 1
                i0, n = (g - g0) * NCAM, run * NCAM  # images of the run, n_img rows of D each
                ops.copy_rows(feats[i0 : i0 + n].view(n * n_img, D), bank[s0 * NCAM : s0 * NCAM + n].view(n * n_img, D))
                g += run
        ep["filled"] = hi

    def _image_slots(self, frame_slots) -> list[list[int]]:
        return [[s * NCAM + c for s in row for c in range(NCAM)] for row in frame_slots]

    def _codes(self, B: int):
        ep = self._ep
        if B not in ep["batch_codes"]:
            ep["batch_codes"][B] = tuple(c.expand(B, -1).contiguous() for c in ep["codes"])
        return ep["batch_codes"][B]

    def _values(self, image_slots, noise, time):
        """kai0_prefix_gather -> embed_suffix -> forward_joint -> value head for len(image_slots) samples -> f32 [n]."""
        from . import ops
        from .model import BF16, F32

        ep, m = self._ep, self.model
        n, Hs = len(image_slots), ep["Hs"]
        prefix = ops.prefix_gather(ep["bank"], image_slots, ep["lang"])
        P, Dp = prefix.shape[1], prefix.shape[2]
        suffix, _, _, cond = m.embed_suffix(None, noise, time)
        De = suffix.shape[2]
        qcode, kcode, pos = self._codes(n)
        out = m.paligemma_with_expert.forward_joint(prefix.view(n * P, Dp), ops.cast(suffix.reshape(n * Hs, De).contiguous(), BF16),
                                                    qcode, kcode, pos, cond, n, P, Hs)  # fmt: skip
        return m._value(ops.cast(out.contiguous(), F32), n, Hs).reshape(n)

    # ---- public ---------------------------------------------------------------------------------------------
    def prefix(self, pass_: int, frame_indices: Sequence[int]):
        """The assembled bf16 prefix [len(frame_indices), P, D] of those samples of the LAST annotated episode's pass (0 = relative,
        1 = absolute), re-running the ring fill for the batches they belong to.  For tests: what `forward_joint` was fed."""
        import torch

        from . import ops

        ep = self._ep
        if ep is None:
            raise RuntimeError("prefix(): annotate an episode first")
        if pass_ not in (0, 1) or (pass_ == 0 and not ep["two"]):
            raise ValueError(f"pass {pass_} does not exist in this episode's mode")
        want = [int(i) for i in frame_indices]
        rows: dict[int, torch.Tensor] = {}
        with torch.no_grad():
            ep["filled"] = 0
            for plan in ep["plans"]:
                self._fill(*plan.fill)
                table = plan.relative_slots if pass_ == 0 else plan.absolute_slots
                hit = [j for j, f in enumerate(plan.frames) if f in want]
                if hit:
                    got = ops.prefix_gather(ep["bank"], self._image_slots([table[j] for j in hit]), ep["lang"])
                    rows.update({plan.frames[j]: got[k].clone() for k, j in enumerate(hit)})
        return torch.stack([rows[i] for i in want])

    def annotate(self, frames, tokens, token_mask, *, two_timesteps: bool = True, relative_interval: int = 50, noise=None, time=None,
                 generator=None) -> dict[str, np.ndarray]:
        """frames: three uint8 arrays [F, H0, W0, 3] (top, left, right); tokens / token_mask: the tokenised prompt [T].
        noise f32 [2, F, H, A] / time f32 [2, F] (pass 0 = relative, 1 = absolute; one-timestep mode reads pass 1 only) may be injected;
        otherwise they are drawn per (pass, frame) from `generator` (a device generator; None: the default one): noise ~ N(0, 1), time ~
        Beta(1.5, 1) * 0.999 + 0.001 as `sample_time` (drawn as U^(1/1.5), the inverse CDF of Beta(a, 1)).
        -> `advantages_from_values`'s fields plus the raw model outputs `raw_absolute` (and `raw_relative`), f32 [F]."""
        import torch

        from .model import F32

        m, dev = self.model, self.device
        if m.training:
            raise ValueError("ValueAnnotator needs the estimator in eval mode (model.eval())")
        with torch.no_grad():
            ep = self._begin(frames, tokens, token_mask, two_timesteps, relative_interval)
            F, Hs, A = ep["F"], ep["Hs"], m.config.action_dim
            if noise is not None and tuple(noise.shape) != (2, F, Hs, A):
                raise ValueError(f"noise must be [2, {F}, {Hs}, {A}], got {tuple(noise.shape)}")
            if time is not None and tuple(time.shape) != (2, F):
                raise ValueError(f"time must be [2, {F}], got {tuple(time.shape)}")
            passes = (0, 1) if two_timesteps else (1,)
            raw = torch.zeros((2, F), dtype=F32)
            for plan in ep["plans"]:
                self._fill(*plan.fill)
                idx = list(plan.frames)
                B = len(idx)
                slots, ns, ts = [], [], []
                for p in passes:
                    slots += self._image_slots(plan.relative_slots if p == 0 else plan.absolute_slots)
                    if noise is not None:
                        ns.append(torch.as_tensor(noise[p, idx[0] : idx[-1] + 1]).to(dev, F32))
                    else:
                        ns.append(torch.randn((B, Hs, A), generator=generator, dtype=F32, device=dev))
                    if time is not None:
                        ts.append(torch.as_tensor(time[p, idx[0] : idx[-1] + 1]).to(dev, F32))
                    else:
                        u = torch.rand((B,), generator=generator, dtype=F32, device=dev)
                        ts.append(u.pow(1.0 / 1.5) * 0.999 + 0.001)
                vals = self._values(slots, torch.cat(ns).contiguous(), torch.cat(ts).contiguous()).cpu()  # the two passes as one batch
                for k, p in enumerate(passes):
                    raw[p, idx[0] : idx[-1] + 1] = vals[k * B : (k + 1) * B]
        raw = raw.numpy()
        out = advantages_from_values(raw[1], raw[0] if two_timesteps else None, relative_interval=relative_interval)
        out["raw_absolute"] = raw[1].copy()
        if two_timesteps:
            out["raw_relative"] = raw[0].copy()
        return out


# ------------------------------------------------------------------------------------------------ dataset loop (eval.py)
def parse_shard(text: str) -> tuple[int, int]:
    i, n = (int(x) for x in text.split("/"))
    if not 0 <= i < n:
        raise ValueError(f"--shard {text}: expected i/n with 0 <= i < n")
    return i, n


def write_annotated_parquet(src_parquet, output_path, columns: dict) -> None:
    """eval.py:107-122: the source table plus the advantage columns it does not have yet."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    table = pq.read_table(src_parquet)
    for name in ADVANTAGE_COLUMNS:
        if name in columns and name not in table.column_names:
            col = np.asarray(columns[name], dtype=np.float64)
            if col.shape[0] != table.num_rows:
                raise ValueError(f"{src_parquet}: {col.shape[0]} values of {name} for {table.num_rows} rows")
            table = table.append_column(name, pa.array(col))
    output_path = pathlib.Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    pq.write_table(table, output_path)


def annotate_dataset(annotator, repo_id, tokens, token_mask, *, name: str, steps: int, two_timesteps: bool = True,
                     relative_interval: int = 50, shard: tuple[int, int] = (0, 1), camera_keys: Sequence[str] = CAMERA_KEYS,
                     frame_decoder: Callable | None = None, tolerance_s: float = 1e-4) -> list[pathlib.Path]:  # fmt: skip
    """eval.py:147-224: every episode of the LeRobot dataset at `repo_id` (paths from meta/info.json) -> a copy of its parquet with
    `relative_advantage`, `absolute_value`, `absolute_advantage` under data_<name>_<steps>/.  Existing outputs and episodes with a
    missing parquet or video are skipped.  `shard` = (i, n): this process takes episodes i, i + n, ... (episodes are independent: no
    collectives).  `frame_decoder(path, timestamps_s, tolerance_s) -> uint8 [T, H, W, 3]`: lerobot_dataset's plug (PyAV, then OpenCV;
    `VideoDecodeUnavailable` where neither is installed).  Returns the files written."""
    import pyarrow.parquet as pq

    from . import lerobot_dataset as lrd

    repo = pathlib.Path(repo_id)
    meta = lrd.LeRobotDatasetMetadata(repo)
    decode = frame_decoder or lrd._default_frame_decoder
    written = []
    for ep in range(shard[0], meta.total_episodes, shard[1]):
        src = meta.data_file(ep)
        if not src.exists():
            logger.warning(f"Parquet file {src} not found, skipping")
            continue
        out = repo / f"data_{name}_{steps}" / src.relative_to(repo / "data")
        if out.exists():
            logger.info(f"Output {out} already exists, skipping")
            continue
        videos = [meta.video_file(ep, k if k in meta.features else f"observation.images.{k}") for k in camera_keys]
        if not all(v.exists() for v in videos):
            logger.warning(f"Missing video file(s) for episode {ep}, skipping")
            continue
        index = pq.read_table(src, columns=["frame_index"])["frame_index"].to_pylist()
        # the evaluator decodes the whole video and slices frames [first, last] of the parquet's frame_index (eval.py:186-188)
        stamps = [i / meta.fps for i in range(int(index[0]), int(index[-1]) + 1)]
        frames = [np.ascontiguousarray(decode(v, stamps, tolerance_s)) for v in videos]
        res = annotator.annotate(frames, tokens, token_mask, two_timesteps=two_timesteps, relative_interval=relative_interval)
        write_annotated_parquet(src, out, res)
        written.append(out)
    return written


# ------------------------------------------------------------------------------------------------ discretize_advantage.py
def get_stage_index(stage_progress_gt: float, stage_nums: int) -> int:
    """discretize_advantage.py:60-79: stage i holds stage_progress_gt in [i / stage_nums, (i + 1) / stage_nums); 1.0 joins the last."""
    if stage_nums == 1:
        return 0
    return min(int(stage_progress_gt / (1.0 / stage_nums)), stage_nums - 1)


def advantage_column(df, advantage_source: str) -> np.ndarray:
    if advantage_source not in ("absolute_advantage", "relative_advantage"):
        raise ValueError(f"Unknown advantage source: {advantage_source}. Must be 'absolute_advantage' or 'relative_advantage'.")
    return df[advantage_source].values.astype(np.float32)


def reward_statistics(rewards) -> dict:
    """discretize_advantage.py:142-175."""
    pts = list(range(0, 101, 10))
    if len(rewards) == 0:
        return {"mean": 0.0, "std": 0.0, "min": 0.0, "max": 0.0, "percentiles": dict.fromkeys(pts, 0.0)}
    r = np.asarray(rewards)
    return {"mean": float(np.mean(r)), "std": float(np.std(r)), "min": float(np.min(r)), "max": float(np.max(r)),
            "percentiles": dict(zip(pts, (float(v) for v in np.percentile(r, pts))))}  # fmt: skip


def binary_threshold(rewards, threshold: float):
    """The advantage above which a frame is labelled positive: the top `threshold` percent (discretize_advantage.py:447-449)."""
    return np.percentile(rewards, 100 - threshold) if len(rewards) else 0.0


def slice_boundaries(rewards, n_slices: int) -> list:
    """The lower edges of `n_slices` equally populated slices (discretize_advantage.py:451-456)."""
    if not len(rewards):
        return [0.0] * n_slices
    step = 100 / n_slices
    return [np.percentile(rewards, step * i) for i in range(n_slices)]


def assign_task_index(rewards: np.ndarray, discretion_type: str, threshold_value=None, boundaries=None, n_slices: int = 10) -> np.ndarray:
    """discretize_advantage.py:233-245 on an array of f32 advantages -> int32 task_index."""
    if discretion_type == "binary":
        return (rewards >= threshold_value).astype(np.int32)
    if discretion_type != "n_slices":
        raise ValueError(f"Unknown discretion_type: {discretion_type}")
    task_index = np.zeros(len(rewards), dtype=np.int32)
    for i in range(len(boundaries) - 1):
        task_index[(rewards >= boundaries[i]) & (rewards < boundaries[i + 1])] = i
    task_index[rewards >= boundaries[-1]] = n_slices - 1
    return task_index


def assign_task_index_staged(rewards: np.ndarray, stage_progress_gt, stage_nums: int, discretion_type: str, thresholds_by_stage=None,
                             boundaries_by_stage=None, n_slices: int = 10) -> np.ndarray:  # fmt: skip
    """discretize_advantage.py:287-310: every frame against the threshold / boundaries of its own stage."""
    stages = np.asarray([get_stage_index(s, stage_nums) for s in stage_progress_gt], dtype=np.int64)
    task_index = np.zeros(len(rewards), dtype=np.int32)
    for st in range(stage_nums):
        sel = stages == st
        if not sel.any():
            continue
        if discretion_type == "binary":
            task_index[sel] = assign_task_index(rewards[sel], "binary", thresholds_by_stage[st])
        elif discretion_type == "n_slices":
            # a frame below the lowest boundary or inside an empty slice keeps 0, as the reference's first-match loop leaves it
            task_index[sel] = assign_task_index(rewards[sel], "n_slices", None, boundaries_by_stage[st], n_slices)
    return task_index


def tasks_for(discretion_type: str, n_slices: int) -> list[dict]:
    """discretize_advantage.py:193-201."""
    if discretion_type == "binary":
        return [{"task_index": 0, "task": "fold the cloth, Advantage: negative"}, {"task_index": 1, "task": "fold the cloth, Advantage: positive"}]
    return [{"task_index": i, "task": f"fold the cloth, Advantage: {i}"} for i in range(n_slices)]


def discretize(data_path, *, threshold: float = 70.0, discretion_type: str = "binary", n_slices: int = 10,
               advantage_source: str = "absolute_advantage", stage_nums: int = 1, dry_run: bool = False) -> dict:  # fmt: skip
    """discretize_advantage.py `main`: statistics of the advantage column over data/chunk-*/*.parquet (per stage of
    `stage_progress_gt` with stage_nums > 1), then — unless `dry_run` — meta/tasks.jsonl rewritten and a `task_index` column written
    into every parquet in place.  Returns {"files", "stats", "thresholds", "boundaries"} (the last three keyed by stage)."""
    import pandas as pd

    if discretion_type not in ("binary", "n_slices"):
        raise ValueError(f"Unknown discretion_type: {discretion_type}")
    base = str(data_path)
    if not os.path.exists(base):
        raise ValueError(f"Path does not exist: {base}")
    pattern = os.path.join(base, "data", "chunk-*", "*.parquet")
    files = sorted(glob.glob(pattern))
    if not files:
        raise ValueError(f"No parquet files found matching pattern: {pattern}")
    by_stage: dict[int, list] = {i: [] for i in range(stage_nums)}
    for f in files:
        df = pd.read_parquet(f)
        rewards = advantage_column(df, advantage_source)
        if stage_nums == 1:
            by_stage[0].extend(rewards.tolist())  # Python floats: the percentiles below are float64 ...
        else:
            if "stage_progress_gt" not in df.columns:
                raise ValueError(f"Column 'stage_progress_gt' not found in {f}. Required when stage_nums > 1.")
            for r, s in zip(rewards, df["stage_progress_gt"].values):
                by_stage[get_stage_index(s, stage_nums)].append(r)  # ... and float32 here, as the reference collects np.float32 scalars
    stats = {st: reward_statistics(r) for st, r in by_stage.items()}
    thresholds = {st: binary_threshold(r, threshold) for st, r in by_stage.items()} if discretion_type == "binary" else {}
    boundaries = {st: slice_boundaries(r, n_slices) for st, r in by_stage.items()} if discretion_type == "n_slices" else {}
    result = {"files": files, "stats": stats, "thresholds": thresholds, "boundaries": boundaries,
              "frames": {st: len(r) for st, r in by_stage.items()}}  # fmt: skip
    if dry_run:
        return result
    os.makedirs(os.path.join(base, "meta"), exist_ok=True)
    with open(os.path.join(base, "meta", "tasks.jsonl"), "w") as fh:
        for task in tasks_for(discretion_type, n_slices):
            fh.write(json.dumps(task) + "\n")
    for f in files:
        df = pd.read_parquet(f)
        rewards = advantage_column(df, advantage_source)
        if stage_nums == 1:
            df["task_index"] = assign_task_index(rewards, discretion_type, thresholds.get(0, 0.0), boundaries.get(0), n_slices)
        else:
            df["task_index"] = assign_task_index_staged(rewards, df["stage_progress_gt"].values, stage_nums, discretion_type, thresholds,
                                                        boundaries, n_slices)  # fmt: skip
        df.to_parquet(f, index=False)
    return result


# ------------------------------------------------------------------------------------------------ CLI
def load_annotator(config_name: str, ckpt_dir: str, *, batch_size: int, siglip_batch: int, trim_prompt: bool, tokenizer_model=None,
                   prompt: str = DEFAULT_PROMPT):  # fmt: skip
    """(ValueAnnotator, tokens, token_mask) for a training config's estimator with `ckpt_dir`/model.safetensors loaded, on cuda:0."""
    import torch

    from .tokenizer import PaligemmaTokenizer
    from .train import build_model
    from .training_config import get_config

    cfg = dataclasses.replace(get_config(config_name), pytorch_weight_path=None)
    from .checkpoint import load_model_safetensors

    model = build_model(cfg, torch.device("cuda:0"))
    load_model_safetensors(model, os.path.join(ckpt_dir, "model.safetensors"), strict=True)
    model.eval()
    tokens, mask = PaligemmaTokenizer(cfg.model.max_token_len, model=tokenizer_model).tokenize(prompt, state=None)
    return ValueAnnotator(model, batch_size=batch_size, siglip_batch=siglip_batch, trim_prompt=trim_prompt), tokens, mask


def main(argv: Sequence[str] | None = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m kai0_amd.stage_advantage", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("annotate", help="write data_<name>_<steps>/ with the estimator's per-frame advantages")
    a.add_argument("repo_id", help="path of the LeRobot dataset")
    a.add_argument("--config", default="ADVANTAGE_TORCH_KAI0_FLATTEN_FOLD", help="training config of the estimator")
    a.add_argument("--ckpt", required=True, help="checkpoint directory holding model.safetensors")
    a.add_argument("--steps", type=int, default=100000, help="checkpoint step, for the output directory's name")
    a.add_argument("--name", default=None, help="output name (default: PI06 with --one-timestep, else KAI0)")
    a.add_argument("--one-timestep", action="store_true", help="PI06: absolute value from the current frame alone")
    a.add_argument("--relative-interval", type=int, default=50)
    a.add_argument("--batch-size", type=int, default=16)
    a.add_argument("--siglip-batch", type=int, default=96)
    a.add_argument("--no-trim-prompt", action="store_true")
    a.add_argument("--prompt", default=DEFAULT_PROMPT)
    a.add_argument("--tokenizer", default=None, help="paligemma sentencepiece model (default: $KAI0_PALIGEMMA_TOKENIZER)")
    a.add_argument("--shard", default="0/1", help="i/n: this process annotates episodes i, i + n, ...")
    d = sub.add_parser("discretize", help="label frames with task_index by advantage percentile")
    d.add_argument("data_path", help="directory holding data/chunk-*/*.parquet")
    d.add_argument("--threshold", type=float, default=70.0, help="top percent labelled positive (binary)")
    d.add_argument("--chunk-size", type=int, default=50, help="unused (kept for the reference's command line)")
    d.add_argument("--discretion-type", default="binary", choices=["binary", "n_slices"])
    d.add_argument("--n-slices", type=int, default=10)
    d.add_argument("--advantage-source", default="absolute_advantage", choices=["absolute_advantage", "relative_advantage"])
    d.add_argument("--stage-nums", type=int, default=1)
    d.add_argument("--dry-run", action="store_true")
    args = ap.parse_args(argv)
    if args.cmd == "discretize":
        res = discretize(args.data_path, threshold=args.threshold, discretion_type=args.discretion_type, n_slices=args.n_slices,
                         advantage_source=args.advantage_source, stage_nums=args.stage_nums, dry_run=args.dry_run)  # fmt: skip
        for st, s in res["stats"].items():
            edge = res["thresholds"].get(st) if args.discretion_type == "binary" else [float(b) for b in res["boundaries"][st]]
            print(f"stage {st}: {res['frames'][st]} frames, mean {s['mean']:.6f} std {s['std']:.6f} min {s['min']:.6f} max {s['max']:.6f}; "
                  f"{'threshold' if args.discretion_type == 'binary' else 'boundaries'} {edge}")  # fmt: skip
        print("dry run: no file modified" if args.dry_run else f"task_index written to {len(res['files'])} files")
        return 0
    two = not args.one_timestep
    annotator, tokens, mask = load_annotator(args.config, args.ckpt, batch_size=args.batch_size, siglip_batch=args.siglip_batch,
                                             trim_prompt=not args.no_trim_prompt, tokenizer_model=args.tokenizer, prompt=args.prompt)  # fmt: skip
    written = annotate_dataset(annotator, args.repo_id, tokens, mask, name=args.name or ("KAI0" if two else "PI06"), steps=args.steps,
                               two_timesteps=two, relative_interval=args.relative_interval, shard=parse_shard(args.shard))  # fmt: skip
    print(f"annotated {len(written)} episodes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
