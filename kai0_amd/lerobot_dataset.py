"""LeRobot-format dataset source for the training loader (`src/openpi/training/data_loader.py:131-228`,
`training/advantage_dataset.py:7-139`): what `create_torch_dataset` / `create_advantage_torch_dataset` hand to the transform
stack — per-frame dictionaries read from a LeRobot v2 dataset directory

    meta/info.json          fps, features {name: {dtype, shape}}, chunks_size, data_path / video_path templates
    meta/tasks.jsonl        {"task_index", "task"}            meta/episodes.jsonl   {"episode_index", "tasks", "length"}
    data/chunk-XXX/episode_YYYYYY.parquet                    one row per frame: state / action vectors, indices, timestamps
    videos/chunk-XXX/<camera>/episode_YYYYYY.mp4             camera streams (AV1); or image columns inside the parquet

with the semantics of `lerobot.common.datasets.lerobot_dataset.LeRobotDataset` (pinned by the reference's uv.lock; restated
here because `lerobot` is not installable offline): `delta_timestamps` turn a key into a stacked window `[T, ...]` clamped to
the episode with a `<key>_is_pad` mask, scalars come back as 0-d tensors, images as float32 CHW in [0, 1], `task` as the
episode's instruction string.

The tabular side is native (pyarrow -> numpy, the whole selected split resident in host memory: 14-DoF x 2 vectors per frame
are ~150 B, i.e. ~0.5 GB per million frames).  Video decoding is a plug: `frame_decoder(path, timestamps_s, tolerance_s)
-> uint8 [T, H, W, 3]`; PyAV / OpenCV are used if importable, and a dataset with video features raises a clear error otherwise
(neither ships in this image).  Image features stored in the parquet (PNG / JPEG bytes) decode with PIL."""

from __future__ import annotations

import dataclasses
import io
import json
import logging
import pathlib
import random
from collections.abc import Callable, Sequence

import numpy as np
import torch

from . import transforms as _transforms

logger = logging.getLogger("kai0_amd")


class VideoDecodeUnavailable(RuntimeError):
    pass


def _read_jsonl(path: pathlib.Path) -> list[dict]:
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


class LeRobotDatasetMetadata:
    """`LeRobotDatasetMetadata(repo_id)` for a local dataset directory (`repo_id` = its path; nothing is downloaded)."""

    def __init__(self, repo_id: str | pathlib.Path, root: str | pathlib.Path | None = None):
        self.repo_id = str(repo_id)
        self.root = pathlib.Path(root if root is not None else repo_id)
        info_path = self.root / "meta" / "info.json"
        if not info_path.exists():
            raise FileNotFoundError(f"{info_path} not found: {self.root} is not a LeRobot v2 dataset directory")
        self.info = json.loads(info_path.read_text())
        self.tasks = {int(t["task_index"]): t["task"] for t in _read_jsonl(self.root / "meta" / "tasks.jsonl")}
        self.episodes = {int(e["episode_index"]): e for e in _read_jsonl(self.root / "meta" / "episodes.jsonl")}

    @property
    def fps(self) -> int:
        return self.info["fps"]

    @property
    def features(self) -> dict:
        return self.info["features"]

    @property
    def video_keys(self) -> list[str]:
        return [k for k, ft in self.features.items() if ft["dtype"] == "video"]

    @property
    def image_keys(self) -> list[str]:
        return [k for k, ft in self.features.items() if ft["dtype"] == "image"]

    @property
    def camera_keys(self) -> list[str]:
        return [k for k, ft in self.features.items() if ft["dtype"] in ("video", "image")]

    @property
    def total_episodes(self) -> int:
        return self.info.get("total_episodes", len(self.episodes))

    def episode_chunk(self, ep: int) -> int:
        return ep // self.info.get("chunks_size", 1000)

    def data_file(self, ep: int) -> pathlib.Path:
        return self.root / self.info["data_path"].format(episode_chunk=self.episode_chunk(ep), episode_index=ep)

    def video_file(self, ep: int, key: str) -> pathlib.Path:
        return self.root / self.info["video_path"].format(episode_chunk=self.episode_chunk(ep), video_key=key, episode_index=ep)


def _default_frame_decoder(path: pathlib.Path, timestamps: Sequence[float], tolerance_s: float) -> np.ndarray:
    """uint8 [T, H, W, 3] frames nearest to `timestamps` (seconds); PyAV first, OpenCV second."""
    try:
        import av  # type: ignore
    except ImportError:
        av = None
    if av is not None:
        with av.open(str(path)) as container:
            stream = container.streams.video[0]
            first, last = min(timestamps), max(timestamps)
            container.seek(int(max(first - 1.0, 0.0) / stream.time_base), stream=stream, backward=True, any_frame=False)
            loaded, ts = [], []
            for frame in container.decode(stream):
                t = float(frame.pts * stream.time_base)
                loaded.append(frame.to_ndarray(format="rgb24"))
                ts.append(t)
                if t >= last:
                    break
        ts = np.asarray(ts)
        idx = [int(np.abs(ts - q).argmin()) for q in timestamps]
        worst = max(abs(ts[i] - q) for i, q in zip(idx, timestamps))
        if worst > tolerance_s:
            raise ValueError(f"{path}: no frame within {tolerance_s}s of the requested timestamps (worst {worst:.4f}s)")
        return np.stack([loaded[i] for i in idx])
    try:
        import cv2  # type: ignore
    except ImportError:
        cv2 = None
    if cv2 is not None:
        cap = cv2.VideoCapture(str(path))
        fps = cap.get(cv2.CAP_PROP_FPS)
        out = []
        for q in timestamps:
            cap.set(cv2.CAP_PROP_POS_FRAMES, round(q * fps))
            ok, frame = cap.read()
            if not ok:
                raise ValueError(f"{path}: cannot decode the frame at {q}s")
            out.append(frame[..., ::-1])
        cap.release()
        return np.stack(out)
    raise VideoDecodeUnavailable(
        f"{path}: this dataset stores its cameras as video, and neither PyAV nor OpenCV is importable. Install one of them, "
        "pass `frame_decoder=` (path, timestamps_s, tolerance_s) -> uint8 [T, H, W, 3], or re-encode the cameras as image "
        "features inside the parquet files.")  # fmt: skip


def get_delta_indices(delta_timestamps: dict[str, list[float]], fps: int, tolerance_s: float = 1e-4) -> dict[str, list[int]]:
    """lerobot `check_delta_timestamps` + `get_delta_indices`: every offset must be a multiple of 1 / fps."""
    out = {}
    for key, deltas in delta_timestamps.items():
        bad = [d for d in deltas if abs(d * fps - round(d * fps)) / fps > tolerance_s]
        if bad:
            raise ValueError(f"delta_timestamps[{key!r}] has values that are not multiples of 1/fps = {1 / fps}: {bad[:4]}")
        out[key] = [round(d * fps) for d in deltas]
    return out


# ------------------------------------------------------------------------------- train-deploy alignment: dataset views
# kai0's `train_deploy_alignment/data_augment` (space_mirroring.py, time_scaling.py) rewrites the dataset on disk: every parquet,
# every video re-encoded with mp4v, the result merged with the original.  Both augmentations are index and column arithmetic on
# data this module already reads, so here they are VIEWS: nothing is written and the frames stay the recorded ones.
# When a config asks for both, time scaling is applied first and mirroring runs over the result (the mirrored half repeats the
# time-scaled sample list).
@dataclasses.dataclass(frozen=True)
class TimeScaling:
    """time_scaling.py: an episode of length L scaled by `factor` N keeps its rows 0, N, 2N, ... (L' = ceil(L / N) frames, frame j
    with frame_index j and timestamp j / fps, every other column and the images from original row j * N; :207,:256,:274-297).
    `split_ratio` (time_scaling_with_split, :435-509): with the episodes sorted by index the first max(1, int(E * split_ratio)) are
    scaled and REPLACE their originals, the rest stay.  Without it every episode is scaled; `union_original` then appends the
    original episodes after the scaled ones, renumbered past them (extract_dataset(..., merge_src_paths=...))."""

    factor: int = 2
    split_ratio: float | None = None
    union_original: bool = False

    def __post_init__(self):
        if isinstance(self.factor, bool) or not isinstance(self.factor, int) or self.factor < 1:
            raise ValueError(f"extraction_factor must be >= 1, got {self.factor}")
        if self.split_ratio is not None and not 0.0 < self.split_ratio < 1.0:
            raise ValueError(f"split_ratio must be between 0 and 1, got {self.split_ratio}")
        if self.split_ratio is not None and self.union_original:
            raise ValueError("split_ratio already keeps the unscaled episodes: union_original goes with split_ratio=None")


@dataclasses.dataclass(frozen=True)
class ViewPlan:
    """Every sample of an augmented dataset as data: the row of the raw state / action tables it starts at, the stride between its
    chunk rows, and whether its arms are swapped.  The one description the loader (`view_plan(dataset)`) and the norm-stats path
    (`plan_view(...)` -> `norm_stats.chunk_rows` / the `_view` kernels) share."""

    frame_idx: np.ndarray  # int32 [M]
    frame_stride: np.ndarray  # int32 [M]
    frame_mirror: np.ndarray  # uint8 [M]

    def __len__(self) -> int:
        return len(self.frame_idx)

    @property
    def is_identity(self) -> bool:
        return bool(np.array_equal(self.frame_idx, np.arange(len(self))) and np.all(self.frame_stride == 1) and not self.frame_mirror.any())


@dataclasses.dataclass(frozen=True)
class _TimePlan:
    rows: np.ndarray  # int64 [M] raw table row of every sample
    stride: np.ndarray  # int32 [M]
    kept: np.ndarray  # int64 [M] index j of the sample among its episode's kept frames; -1: a sample of an unscaled episode
    ep_shift: np.ndarray  # int64 [M] added to episode_index
    num_episodes: int  # episodes of the view


def scaled_episode_positions(episode_ids: Sequence[int], ts: TimeScaling) -> list[int]:
    """Positions (in `episode_ids`' order) of the episodes a TimeScaling scales."""
    if ts.split_ratio is None:
        return list(range(len(episode_ids)))
    order = sorted(range(len(episode_ids)), key=lambda p: int(episode_ids[p]))
    return sorted(order[: max(1, int(len(episode_ids) * ts.split_ratio))])


def _time_plan(lengths: Sequence[int], episode_ids: Sequence[int], ts: TimeScaling | None) -> _TimePlan:
    lengths = [int(n) for n in lengths]
    starts = np.cumsum([0, *lengths])[:-1]
    scaled = set(scaled_episode_positions(episode_ids, ts)) if ts is not None else set()
    parts = []  # (rows, stride, kept, ep_shift)
    passes = [(True, 0), (False, len(lengths))] if ts is not None and ts.union_original else [(None, 0)]
    for only_scaled, shift in passes:
        for p, (s0, n) in enumerate(zip(starts, lengths, strict=True)):
            if (p in scaled) if only_scaled is None else only_scaled:
                rows = s0 + np.arange(0, n, ts.factor, dtype=np.int64)
                parts.append((rows, np.full(len(rows), ts.factor), np.arange(len(rows)), np.full(len(rows), shift)))
            else:
                rows = s0 + np.arange(n, dtype=np.int64)
                parts.append((rows, np.ones(n), np.full(n, -1), np.full(n, shift)))
    cat = [np.concatenate([p[k] for p in parts]) if parts else np.zeros(0) for k in range(4)]
    return _TimePlan(cat[0].astype(np.int64), cat[1].astype(np.int32), cat[2].astype(np.int64), cat[3].astype(np.int64),
                     len(lengths) * len(passes))  # fmt: skip


def plan_view(lengths: Sequence[int], episode_ids: Sequence[int] | None = None, time_scaling: TimeScaling | None = None,
              space_mirror: bool = False) -> ViewPlan:  # fmt: skip
    """The ViewPlan of a dataset whose episodes (in the dataset's order) have these lengths, under the augmentations of a data
    config: time scaling first, then original ∪ mirrored."""
    tp = _time_plan(lengths, episode_ids if episode_ids is not None else list(range(len(lengths))), time_scaling)
    reps = 2 if space_mirror else 1
    mirror = np.repeat(np.arange(reps, dtype=np.uint8), len(tp.rows))
    return ViewPlan(np.tile(tp.rows, reps).astype(np.int32), np.tile(tp.stride, reps).astype(np.int32), mirror)


class LeRobotDataset:
    """Map-style dataset of frames (see the module docstring).  `episodes`: subset, in this order (default: all).
    `time_scaling`: a TimeScaling; the samples are then the kept frames (and the action windows step through the kept frames)."""

    def __init__(self, repo_id: str | pathlib.Path, root: str | pathlib.Path | None = None, episodes: list[int] | None = None,
                 image_transforms: Callable | None = None, delta_timestamps: dict[str, list[float]] | None = None,
                 tolerance_s: float = 1e-4, frame_decoder: Callable | None = None, time_scaling: TimeScaling | None = None,
                 **_ignored):  # fmt: skip
        import pyarrow.parquet as pq

        self.repo_id = str(repo_id)
        self.meta = LeRobotDatasetMetadata(repo_id, root)
        self.root = self.meta.root
        self.episodes = list(episodes) if episodes is not None else None
        self.image_transforms = image_transforms
        self.tolerance_s = tolerance_s
        self.frame_decoder = frame_decoder or _default_frame_decoder
        self.delta_timestamps = delta_timestamps
        self.delta_indices = get_delta_indices(delta_timestamps, self.meta.fps, tolerance_s) if delta_timestamps else None
        eps = self.episodes if self.episodes is not None else sorted(self.meta.episodes)
        tables = []
        lengths = []
        for ep in eps:
            t = pq.read_table(self.meta.data_file(ep))
            tables.append(t)
            lengths.append(t.num_rows)
        import pyarrow as pa

        table = pa.concat_tables(tables) if tables else None
        self._columns: dict[str, np.ndarray | list] = {}
        self._image_cols: dict[str, list] = {}
        for name in (table.column_names if table is not None else []):
            ft = self.meta.features.get(name, {})
            col = table.column(name)
            if ft.get("dtype") == "image":
                self._image_cols[name] = col.to_pylist()  # {"bytes": ..., "path": ...} per frame
                continue
            arr = col.to_numpy(zero_copy_only=False) if not pa.types.is_list(col.type) and not pa.types.is_fixed_size_list(col.type) else None
            if arr is None:
                arr = np.stack([np.asarray(x) for x in col.to_pylist()]) if len(col) else np.zeros((0,))
            if arr.dtype == np.float64 and ft.get("dtype") == "float32":
                arr = arr.astype(np.float32)
            self._columns[name] = arr
        ends = np.cumsum(lengths)
        self.episode_data_index = {"from": torch.as_tensor(ends - np.asarray(lengths), dtype=torch.int64),
                                   "to": torch.as_tensor(ends, dtype=torch.int64)}  # fmt: skip
        self._ep_pos = {ep: i for i, ep in enumerate(eps)}  # episode index -> position in episode_data_index
        self._num_frames = int(ends[-1]) if len(ends) else 0
        self.time_scaling = time_scaling
        # None without time scaling: every sample is its table row and nothing below takes another path
        self._view = _time_plan(lengths, eps, time_scaling) if time_scaling is not None else None

    # ------------------------------------------------------------------------------------------------ LeRobotDataset API
    @property
    def fps(self) -> int:
        return self.meta.fps

    @property
    def num_frames(self) -> int:
        return self._num_frames

    @property
    def num_episodes(self) -> int:
        return len(self._ep_pos)

    @property
    def num_view_episodes(self) -> int:
        """Episodes of the view: twice num_episodes where the originals are appended to their time-scaled copies."""
        return self._view.num_episodes if self._view is not None else self.num_episodes

    def __len__(self) -> int:
        return len(self._view.rows) if self._view is not None else self._num_frames

    def _locate(self, idx: int) -> tuple[int, tuple[int, int] | None]:
        """Sample -> (table row, None) or, for a frame of a time-scaled episode, (table row, (kept index j, factor N))."""
        if self._view is None:
            return idx, None
        j = int(self._view.kept[idx])
        return int(self._view.rows[idx]), ((j, int(self._view.stride[idx])) if j >= 0 else None)

    def _restamp(self, item: dict, idx: int, scaled: tuple[int, int] | None, prefix: str = "") -> None:
        """What extraction rewrites in a kept row (time_scaling.py:274-297): frame_index j, timestamp j / fps; and the episode
        number a merge gives the appended originals."""
        if scaled is not None:
            for key, value in (("frame_index", scaled[0]), ("timestamp", scaled[0] / self.fps)):
                if prefix + key in item:
                    item[prefix + key] = torch.as_tensor(np.asarray(value, dtype=self._columns[key].dtype))
        shift = int(self._view.ep_shift[idx]) if self._view is not None else 0
        if shift and prefix + "episode_index" in item:
            item[prefix + "episode_index"] = item[prefix + "episode_index"] + shift

    def _row(self, idx: int) -> dict:
        item = {}
        for k, arr in self._columns.items():
            item[k] = torch.as_tensor(np.asarray(arr[idx]))
        return item

    def _get_query_indices(self, idx: int, ep_pos: int, scaled: tuple[int, int] | None = None):
        start, end = int(self.episode_data_index["from"][ep_pos]), int(self.episode_data_index["to"][ep_pos])
        if scaled is not None:  # lerobot's window clamp on the shortened episode: row h is kept frame min(j + h, L' - 1)
            j, n = scaled
            kept = -(-(end - start) // n)
            query = {k: [start + max(0, min(kept - 1, j + d)) * n for d in deltas] for k, deltas in self.delta_indices.items()}
            padding = {f"{k}_is_pad": torch.BoolTensor([(j + d < 0) | (j + d > kept - 1) for d in deltas])
                       for k, deltas in self.delta_indices.items()}  # fmt: skip
            return query, padding
        query = {k: [max(start, min(end - 1, idx + d)) for d in deltas] for k, deltas in self.delta_indices.items()}
        padding = {f"{k}_is_pad": torch.BoolTensor([(idx + d < start) | (idx + d >= end) for d in deltas])
                   for k, deltas in self.delta_indices.items()}  # fmt: skip
        return query, padding

    def _query_hf_dataset(self, query_indices: dict[str, list[int]]) -> dict:
        out = {}
        for k, q in query_indices.items():
            if k in self.meta.video_keys:
                continue
            if k in self._image_cols:
                out[k] = torch.stack([self._decode_image(self._image_cols[k][i]) for i in q])
            else:
                out[k] = torch.as_tensor(np.stack([np.asarray(self._columns[k][i]) for i in q]))
        return out

    @staticmethod
    def _decode_image(cell) -> torch.Tensor:
        from PIL import Image

        raw = cell["bytes"] if isinstance(cell, dict) else cell
        img = np.array(Image.open(io.BytesIO(raw)).convert("RGB"))
        return torch.from_numpy(img).permute(2, 0, 1).to(torch.float32) / 255.0  # CHW in [0, 1], as lerobot's hf_transform

    def _query_videos(self, query_timestamps: dict[str, list[float]], ep: int) -> dict:
        out = {}
        for k, ts in query_timestamps.items():
            frames = self.frame_decoder(self.meta.video_file(ep, k), ts, self.tolerance_s)
            t = torch.from_numpy(np.ascontiguousarray(frames)).permute(0, 3, 1, 2).to(torch.float32) / 255.0
            out[k] = t.squeeze(0) if t.shape[0] == 1 else t
        return out

    def _get_query_timestamps(self, current_ts: float, query_indices: dict | None) -> dict[str, list[float]]:
        out = {}
        for k in self.meta.video_keys:
            if query_indices is not None and k in query_indices:
                out[k] = [float(self._columns["timestamp"][i]) for i in query_indices[k]]
            else:
                out[k] = [current_ts]
        return out

    def get_sample_with_imgs_from_idx(self, idx: int) -> dict:
        """One frame with its cameras decoded (no action window)."""
        item = self._row(idx)
        ep = int(item["episode_index"])
        for k, cells in self._image_cols.items():
            item[k] = self._decode_image(cells[idx])
        if self.meta.video_keys:
            item = {**self._query_videos(self._get_query_timestamps(float(item["timestamp"]), None), ep), **item}
        if self.image_transforms is not None:
            for cam in self.meta.camera_keys:
                item[cam] = self.image_transforms(item[cam])
        return item

    def __getitem__(self, idx: int) -> dict:
        if idx < 0:
            idx += len(self)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        sample = idx
        idx, scaled = self._locate(sample)  # from here on idx is the table row: the recorded frame
        item = self._row(idx)
        ep = int(item["episode_index"])
        query_indices = None
        if self.delta_indices is not None:
            query_indices, padding = self._get_query_indices(idx, self._ep_pos[ep], scaled)
            item = {**item, **padding, **self._query_hf_dataset(query_indices)}
        for k, cells in self._image_cols.items():
            if query_indices is None or k not in query_indices:
                item[k] = self._decode_image(cells[idx])
        if self.meta.video_keys:
            frames = self._query_videos(self._get_query_timestamps(float(item["timestamp"]), query_indices), ep)
            item = {**frames, **item}
        if self.image_transforms is not None:
            for cam in self.meta.camera_keys:
                item[cam] = self.image_transforms(item[cam])
        item["task"] = self.meta.tasks[int(item["task_index"])]
        self._restamp(item, sample, scaled)
        return item


class AdvantageLerobotDataset(LeRobotDataset):
    """`training/advantage_dataset.py:7-139`: every sample also carries a RANDOM other frame of the same episode under
    `his_-100_<key>` and the label `progress = stage_progress_gt - his_-100_stage_progress_gt` (Stage-Advantage estimator)."""

    def __getitem__(self, idx: int) -> dict:
        if idx < 0:
            idx += len(self)
        sample = idx
        idx, scaled = self._locate(sample)  # from here on idx is the table row
        item = self.get_sample_with_imgs_from_idx(idx)
        ep = int(item["episode_index"])
        ts = float(item["timestamp"])
        pos = self._ep_pos[ep]
        start, end = int(self.episode_data_index["from"][pos]), int(self.episode_data_index["to"][pos])
        kept = -(-(end - start) // scaled[1]) if scaled is not None else None  # L' of a time-scaled episode
        level = {"episode_length": self.meta.episodes[ep]["length"] if scaled is None else kept}
        if self.delta_indices is not None:
            query_indices, padding = self._get_query_indices(idx, self._ep_pos[ep], scaled)
            level = {**level, **padding, **self._query_hf_dataset(query_indices)}
        level["task"] = self.meta.tasks[int(item["task_index"])]
        if (end - start if scaled is None else kept) < 2:
            raise ValueError(f"episode {ep} has a single frame: no comparison frame to draw")
        while True:
            if scaled is None:
                j = random.randint(start, end - 1)
            else:  # the other frame is one of the kept ones
                other_kept = random.randint(0, kept - 1)
                j = start + other_kept * scaled[1]
            if j == idx:
                continue
            other = self.get_sample_with_imgs_from_idx(j)
            if int(other["episode_index"]) == ep and float(other["timestamp"]) != ts:
                break
        other = {f"his_-100_{k}": v for k, v in other.items()}
        self._restamp(item, sample, scaled)
        self._restamp(other, sample, (other_kept, scaled[1]) if scaled is not None else None, prefix="his_-100_")
        final = {**other, **item, **level}
        final["progress"] = float(final["stage_progress_gt"]) - float(final["his_-100_stage_progress_gt"])
        return final


# ------------------------------------------------------------------------------------------- space_mirroring.py
HIS_PREFIX = "his_-100_"  # AdvantageLerobotDataset's comparison frame: mirrored with the sample it belongs to


def camera_mirror_map(camera_keys: Sequence[str], flip_only: Sequence[str] = ()) -> dict[str, str]:
    """Camera key of the mirrored sample -> the camera whose flipped frame it shows (space_mirroring.py:524-560): `top_head` from
    itself, `hand_left` from `hand_right` and back.  A camera that is none of the three roles must be named in `flip_only` (the
    reference drops its videos without a word; here it is an error)."""
    out = {}
    for key in camera_keys:
        role = key.rpartition(".")[2]
        if role == "top_head" or key in flip_only or role in flip_only:
            out[key] = key
        elif role in ("hand_left", "hand_right"):
            out[key] = key[: len(key) - len(role)] + ("hand_right" if role == "hand_left" else "hand_left")
            if out[key] not in camera_keys:
                raise ValueError(f"space mirroring: camera {key!r} has no counterpart {out[key]!r} in the dataset")
        else:
            raise ValueError(f"space mirroring: camera {key!r} is neither top_head, hand_left nor hand_right; "
                             "name it in flip_only to flip it in place")  # fmt: skip
    return out


def _base_dataset(dataset):
    """The LeRobotDataset under the views wrapped around it."""
    while not isinstance(dataset, LeRobotDataset):
        inner = next((v for v in (getattr(dataset, "dataset", None), getattr(dataset, "_dataset", None),
                                  getattr(dataset, "datasets", [None])[0]) if v is not None), None)  # fmt: skip
        if inner is None:
            raise TypeError(f"{type(dataset).__name__} is not a view over a LeRobotDataset")
        dataset = inner
    return dataset


class MirroredView:
    """The left-right mirrored twin of a LeRobotDataset / AdvantageLerobotDataset (or of a view over one), sample by sample
    (space_mirroring.py): vectors of exactly left_dim + right_dim values under `vector_keys` become [right, left] (no sign change,
    any other length is a ValueError), every camera is flipped left-right and the two hand cameras trade places, and the same is
    done to the `his_-100_*` copy the Stage-Advantage dataset carries.  progress, task, timestamps, indices and the pad flags are
    the original's; `episode_offset` is added to episode_index (a merge renumbers the mirrored episodes past the originals).
    The swap is on the RAW sample, before repack and every transform: where the mirrored parquet would be.  Time scaling, if
    any, has already happened inside `dataset`."""

    def __init__(self, dataset, left_dim: int = 7, right_dim: int = 7, *, vector_keys: Sequence[str] = ("observation.state", "action"),
                 flip_only: Sequence[str] = (), episode_offset: int = 0):  # fmt: skip
        self.dataset = dataset
        self.left_dim, self.right_dim = int(left_dim), int(right_dim)
        self.vector_keys = tuple(vector_keys)
        self.episode_offset = int(episode_offset)
        self.meta = _base_dataset(dataset).meta
        self._cameras = camera_mirror_map(self.meta.camera_keys, flip_only)

    def __len__(self) -> int:
        return len(self.dataset)

    def mirror_sample(self, item: dict) -> dict:
        from .normalize import swap_arms

        out = dict(item)
        for key, value in item.items():
            prefix = HIS_PREFIX if key.startswith(HIS_PREFIX) else ""
            base = key[len(prefix) :]
            if base in self.vector_keys:
                out[key] = swap_arms(value, self.left_dim, self.right_dim)
            elif base in self._cameras:
                out[key] = torch.flip(item[prefix + self._cameras[base]], dims=[-1])  # [..., H, W]: cv2.flip(frame, 1)
            elif base == "episode_index" and self.episode_offset:
                out[key] = value + self.episode_offset
        return out

    def __getitem__(self, idx: int) -> dict:
        return self.mirror_sample(self.dataset[idx])


class ConcatView:
    """Datasets one after another (the merge of space_mirroring.py's `full` command, as an index map)."""

    def __init__(self, datasets: Sequence):
        self.datasets = list(datasets)
        self._ends = np.cumsum([len(d) for d in self.datasets])
        self.meta = _base_dataset(self.datasets[0]).meta

    def __len__(self) -> int:
        return int(self._ends[-1])

    def __getitem__(self, idx: int) -> dict:
        if idx < 0:
            idx += len(self)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        k = int(np.searchsorted(self._ends, idx, side="right"))
        return self.datasets[k][idx - (int(self._ends[k - 1]) if k else 0)]


def with_mirror(dataset, left_dim: int = 7, right_dim: int = 7, **kw) -> ConcatView:
    """original ∪ mirrored: 2 * len(dataset) samples, sample i < len the original, i >= len the mirrored sample i - len with its
    episode_index moved past the dataset's episodes."""
    return ConcatView([dataset, MirroredView(dataset, left_dim, right_dim, episode_offset=_base_dataset(dataset).num_view_episodes, **kw)])


def view_plan(dataset) -> ViewPlan:
    """The ViewPlan of a dataset as the loader sees it: a LeRobotDataset (time-scaled or not) under any nesting of MirroredView,
    ConcatView / with_mirror and TransformedDataset."""
    if isinstance(dataset, LeRobotDataset):
        if dataset._view is None:
            n = len(dataset)
            return ViewPlan(np.arange(n, dtype=np.int32), np.ones(n, np.int32), np.zeros(n, np.uint8))
        return ViewPlan(dataset._view.rows.astype(np.int32), dataset._view.stride.copy(), np.zeros(len(dataset), np.uint8))
    if isinstance(dataset, MirroredView):
        p = view_plan(dataset.dataset)
        return ViewPlan(p.frame_idx, p.frame_stride, (p.frame_mirror ^ 1).astype(np.uint8))
    if isinstance(dataset, ConcatView):
        parts = [view_plan(d) for d in dataset.datasets]
        return ViewPlan(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("frame_idx", "frame_stride", "frame_mirror")))
    if hasattr(dataset, "_dataset"):  # TransformedDataset
        return view_plan(dataset._dataset)
    raise TypeError(f"{type(dataset).__name__} is not a view over a LeRobotDataset")


def _view_kw(data_config) -> dict:
    """Nothing for a config without time scaling: the dataset is then constructed exactly as before."""
    ts = getattr(data_config, "time_scaling", None)
    return {} if ts is None else {"time_scaling": ts}


def _augmented(dataset, data_config):
    """`space_mirror` of a data config over a dataset that already carries its `time_scaling`."""
    if not getattr(data_config, "space_mirror", False):
        return dataset
    keys = ("observation.state", "action")
    for t in data_config.repack_transforms.inputs:  # the raw columns the config calls "state" and "actions"
        if isinstance(t, _transforms.RepackTransform) and all(isinstance(t.structure.get(k), str) for k in ("state", "actions")):
            keys = (t.structure["state"], t.structure["actions"])
    return with_mirror(dataset, data_config.left_dim, data_config.right_dim, vector_keys=keys, flip_only=tuple(data_config.mirror_flip_only))


# ------------------------------------------------------------------------------------------- data_loader.py:131-228
def episodes_split_through_task(repo_id, split_ratio: float = 0.9, split_type: str = "train", shuffle: bool = False,
                                random_seed: int = 42) -> list[int]:  # fmt: skip
    """data_loader.py:185-213: per task, the first `split_ratio` of its episodes train, the rest validate."""
    assert split_type in ["all", "train", "val"], f"Invalid split type '{split_type}'. Must be 'all', 'train' or 'val'."
    meta = LeRobotDatasetMetadata(repo_id)
    index = list(meta.episodes.keys())
    if split_type == "all":
        return index
    by_task: dict[str, list[int]] = {}
    for i in index:
        by_task.setdefault("".join(meta.episodes[i]["tasks"]), []).append(i)
    train, val = [], []
    for eps in by_task.values():
        n = int(len(eps) * split_ratio)
        train.extend(eps[:n])
        val.extend(eps[n:])
    return train if split_type == "train" else val


def create_torch_dataset(data_config, action_horizon: int, model_config, **dataset_kw):
    """data_loader.py:131-152."""
    from .data_loader import FakeDataset, TransformedDataset

    repo_id = data_config.repo_id
    if repo_id is None:
        raise ValueError("Repo ID is not set. Cannot create dataset.")
    if repo_id == "fake":
        return FakeDataset(model_config, num_samples=1024)
    meta = LeRobotDatasetMetadata(repo_id)
    dataset = LeRobotDataset(
        repo_id, episodes=getattr(data_config, "episodes", None),
        delta_timestamps={key: [t / meta.fps for t in range(action_horizon)] for key in data_config.action_sequence_keys},
        **_view_kw(data_config), **dataset_kw)  # fmt: skip
    dataset = _augmented(dataset, data_config)
    if data_config.prompt_from_task:
        dataset = TransformedDataset(dataset, [_transforms.PromptFromLeRobotTask(meta.tasks)])
    return dataset


def create_advantage_torch_dataset(data_config, action_horizon: int, model_config, config=None, **dataset_kw):
    """data_loader.py:154-182."""
    from .data_loader import FakeDataset, TransformedDataset

    split = getattr(config, "split", "all") or "all"
    repo_id = data_config.repo_id
    if repo_id is None:
        raise ValueError("Repo ID is not set. Cannot create dataset.")
    if repo_id == "fake":
        return FakeDataset(model_config, num_samples=1024)
    meta = LeRobotDatasetMetadata(repo_id)
    dataset = AdvantageLerobotDataset(
        repo_id, episodes=episodes_split_through_task(repo_id, split_type=split, shuffle=False),
        delta_timestamps={key: [t / meta.fps for t in range(action_horizon)] for key in data_config.action_sequence_keys},
        **_view_kw(data_config), **dataset_kw)  # fmt: skip
    dataset = _augmented(dataset, data_config)
    if data_config.prompt_from_task:
        dataset = TransformedDataset(dataset, [_transforms.PromptFromLeRobotTask(meta.tasks)])
    return dataset


def read_state_action_columns(repo_id, state_col: str, action_col: str, episodes: list[int] | None = None):
    """The two vector columns of a dataset and its episode boundaries, for `kai0_amd.norm_stats`: f32 [N, ds], f32 [N, da] and
    int32 ep_end [N] (ep_end[i] = one past the last row of frame i's episode), episodes in `LeRobotDataset`'s order.  Only these two
    columns are read from each parquet file: image columns and videos are never touched."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    meta = LeRobotDatasetMetadata(repo_id)
    eps = list(episodes) if episodes is not None else sorted(meta.episodes)
    parts: dict[str, list[np.ndarray]] = {state_col: [], action_col: []}
    lengths = []
    for ep in eps:
        t = pq.read_table(meta.data_file(ep), columns=[state_col, action_col])
        lengths.append(t.num_rows)
        for name in (state_col, action_col):
            col = t.column(name).combine_chunks()
            if pa.types.is_list(col.type) or pa.types.is_large_list(col.type) or pa.types.is_fixed_size_list(col.type):
                flat = col.flatten().to_numpy(zero_copy_only=False)
                if t.num_rows and (flat.size % t.num_rows or col.null_count):
                    raise ValueError(f"{meta.data_file(ep)}: column {name!r} is not a table of equally long vectors")
                arr = flat.reshape(t.num_rows, -1) if t.num_rows else flat.reshape(0, 0)
            else:
                arr = col.to_numpy(zero_copy_only=False).reshape(t.num_rows, 1)
            parts[name].append(arr.astype(np.float32, copy=False))
    widths = {name: {a.shape[1] for a in arrs if len(a)} for name, arrs in parts.items()}
    if any(len(w) > 1 for w in widths.values()):
        raise ValueError(f"{meta.root}: the width of {state_col!r} / {action_col!r} changes between episodes: {widths}")
    state, action = (np.concatenate([a for a in parts[name] if len(a)]) if any(len(a) for a in parts[name]) else np.zeros((0, 0), np.float32)
                     for name in (state_col, action_col))  # fmt: skip
    ep_end = np.repeat(np.cumsum(lengths), lengths).astype(np.int32)
    return state, action, ep_end


def transform_dataset(dataset, data_config, *, skip_norm_stats: bool = False):
    """data_loader.py:230-251: repack -> robot transforms -> Normalize -> model transforms."""
    from .data_loader import TransformedDataset

    norm_stats = {}
    if data_config.repo_id != "fake" and not skip_norm_stats:
        if data_config.norm_stats is None:
            raise ValueError("Normalization stats not found. Make sure to run `python -m kai0_amd.compute_norm_stats <your-config>`.")
        norm_stats = data_config.norm_stats
    return TransformedDataset(dataset, [*data_config.repack_transforms.inputs, *data_config.data_transforms.inputs,
                                        _transforms.Normalize(norm_stats, use_quantiles=data_config.use_quantile_norm),
                                        *data_config.model_transforms.inputs])  # fmt: skip


def create_data_loader(config, *, shuffle: bool = False, num_batches: int | None = None, skip_norm_stats: bool = False,
                       framework: str = "pytorch", **dataset_kw):  # fmt: skip
    """`create_data_loader(train_config)` (data_loader.py:291-330, torch path): TrainConfig -> dataset -> transforms -> batches of
    `(Observation, actions)`; under torch.distributed every rank gets batch_size / world_size samples of its own shard."""
    from .data_loader import create_torch_data_loader

    if framework != "pytorch":
        raise ValueError("kai0_amd loads data for the torch path only")
    data_config = config.data.create(config.assets_dirs, config.model)
    logger.info(f"data_config: {data_config}")
    if getattr(config, "advantage_estimator", False):
        dataset = create_advantage_torch_dataset(data_config, config.model.action_horizon, config.model, config, **dataset_kw)
    else:
        dataset = create_torch_dataset(data_config, config.model.action_horizon, config.model, **dataset_kw)
    dataset = transform_dataset(dataset, data_config, skip_norm_stats=skip_norm_stats or getattr(config, "skip_norm_stats", False))
    return create_torch_data_loader(dataset, config.batch_size, shuffle=shuffle, num_batches=num_batches,
                                    num_workers=config.num_workers, seed=config.seed, data_config=data_config)  # fmt: skip
