"""Normalisation statistics of a dataset (`assets/<asset_id>/norm_stats.json`) — the step between a new task directory and `train`:
what `scripts/compute_norm_stats.py` of the reference computes (:102-109: every transformed sample's "state" and "actions" through
`normalize.RunningStats`), without pulling a single frame through the data loader.

The statistic covers N x action_horizon x action_dim virtual elements, yet every one of them is a function of two small tables (the
state and action columns of the parquet files) and the episode boundaries.  So the robot transforms of a data config are LOWERED
(`lower_transforms`) to a `ChunkSpec` — which columns, which glitch filters, which delta mask — and the statistic is computed from the
tables: on the GPU by two HIP passes (`kai0_chunk_stats_moments`, `kai0_chunk_stats_hist`; csrc/norm_stats.hip) that gather the
chunk rows on the fly, on the host by `chunk_rows`, the numpy restatement of the same transform stack (tests/test_norm_stats_cpu.py
holds it to `TransformedDataset` bit for bit).  Cameras are never decoded.  A transform stack that cannot be lowered still gets its
file: the reference's loop over the transformed dataset.

The estimator is the one this repository pins to the reference (tests/golden/normalize_golden.json), in its ONE-SHOT form:
`RunningStats().update(rows.astype(np.float64))` once per key — edges `np.linspace(lo - 1e-10, hi + 1e-10, 5001)`, `np.histogram`'s
counts, quantile `edges[searchsorted(cumsum(hist), q * count)]`.  The reference's script streams batches of 32 through the same class,
which re-bins the histogram whenever the range grows; the two differ by that re-binning smear only."""

from __future__ import annotations

import dataclasses
import logging
import pathlib

import numpy as np

from . import agilex_policy
from . import normalize as _normalize
from . import transforms as _transforms
from .normalize import QUANTILE_BINS, NormStats, RunningStats

logger = logging.getLogger("kai0_amd")

PI_F32 = np.float32(np.pi)  # `np.abs(x) > np.pi` on an f32 array compares with f32(pi): x == f32(pi) is kept
MAX_WIDTH = 32  # columns one kernel launch takes (a 32-bit delta mask)
HOST_SLAB_ROWS = 1 << 22  # virtual rows (frames x horizon) the host path materialises at a time
KEYS = ("state", "actions")


@dataclasses.dataclass(frozen=True)
class ChunkSpec:
    """What `repack_transforms.inputs + data_transforms.inputs` do to "state" and "actions", as data."""

    state_col: str
    action_col: str
    action_dim: int
    clip_state: bool
    clip_action: bool
    mask_state: bool
    delta_mask: int  # bit c: actions[..., c] -= state[c]


def mask_bits(mask) -> int:
    return sum(1 << c for c, m in enumerate(mask or ()) if m)


def lower_transforms(data_config) -> ChunkSpec | None:
    """The input transform stack of a DataConfig as a ChunkSpec, or None where it holds anything but: one RepackTransform naming
    the two columns, one AgilexInputs / ARXInputs, InsertAdvantageIntoPrompt (which touches neither key), at most one DeltaActions
    after the inputs class."""
    cols = inputs = None
    delta = 0
    seen_delta = False
    for t in (*data_config.repack_transforms.inputs, *data_config.data_transforms.inputs):
        if type(t) is _transforms.RepackTransform:
            s, a = t.structure.get("state"), t.structure.get("actions")
            if cols is not None or inputs is not None or not isinstance(s, str) or not isinstance(a, str):
                return None
            cols = (s, a)
        elif type(t) in (agilex_policy.AgilexInputs, agilex_policy.ARXInputs):
            if cols is None or inputs is not None:
                return None
            inputs = t
        elif type(t) is _transforms.InsertAdvantageIntoPrompt:
            continue
        elif type(t) is _transforms.DeltaActions:
            if inputs is None or seen_delta:
                return None
            seen_delta = True
            if t.mask is not None:
                if len(t.mask) > inputs.action_dim:
                    return None
                delta = mask_bits(t.mask)
        else:
            return None
    if cols is None or inputs is None or not 1 <= inputs.action_dim <= MAX_WIDTH:
        return None
    if cols[1] not in tuple(data_config.action_sequence_keys):  # the action column must come back as a window
        return None
    return ChunkSpec(state_col=cols[0], action_col=cols[1], action_dim=inputs.action_dim, clip_state=type(inputs).filter_state_glitches,
                     clip_action=True, mask_state=bool(inputs.mask_state), delta_mask=delta)  # fmt: skip


def _clip(x: np.ndarray) -> np.ndarray:
    return np.where(np.abs(x) > PI_F32, np.float32(0), x)


def _pad(x: np.ndarray, dim: int) -> np.ndarray:
    if x.shape[-1] > dim:
        raise ValueError(f"a table of {x.shape[-1]} columns does not fit action_dim = {dim}")
    return _transforms.pad_to_dim(x, dim)


def chunk_rows(state, action, ep_end, *, horizon: int, action_dim: int, clip_state: bool, clip_action: bool, mask_state: bool,
               delta_mask: int, frame_idx=None, frame_stride=None, frame_mirror=None, left_dim: int = 7,
               right_dim: int = 7) -> tuple[np.ndarray, np.ndarray]:  # fmt: skip
    """What the transformed dataset yields under "state" and "actions" for the frames `frame_idx` (default: all), from the tables:
    f32 [M, action_dim] and f32 [M, horizon, action_dim].  state [N, ds] / action [N, da] f32, ep_end[i] = one past the last row of
    frame i's episode: chunk row h of frame i is action row min(i + h, ep_end[i] - 1).
    A dataset view (`lerobot_dataset.ViewPlan`) adds, per frame, `frame_stride` s (time scaling: chunk row h is row
    min(i + h s, last kept row of the episode), the kept rows being i, i + s, ...) and `frame_mirror` (space mirroring: the first
    left_dim + right_dim columns of the padded state and action rows become [right, left] BEFORE the glitch filter, the state
    mask and the delta subtraction — where a mirrored parquet would have them).  With both None this is the plain function."""
    state, action = np.asarray(state, np.float32), np.asarray(action, np.float32)
    ep_end = np.asarray(ep_end, np.int64)
    idx = np.arange(len(state)) if frame_idx is None else np.asarray(frame_idx, np.int64)
    if frame_stride is None:
        rows = np.minimum(idx[:, None] + np.arange(horizon)[None, :], ep_end[idx][:, None] - 1)
    else:
        step = np.maximum(np.asarray(frame_stride, np.int64), 1)
        last = idx + (ep_end[idx] - 1 - idx) // step * step
        rows = np.minimum(idx[:, None] + np.arange(horizon)[None, :] * step[:, None], last[:, None])
    s = _pad(state[idx], action_dim)
    a = _pad(action[rows], action_dim)
    if frame_mirror is not None:
        perm = _normalize.arm_swap_perm(action_dim, left_dim, right_dim)
        flip = np.asarray(frame_mirror).astype(bool)
        s = np.where(flip[:, None], s[:, perm], s)
        a = np.where(flip[:, None, None], a[:, :, perm], a)
    if clip_state:
        s = _clip(s)
    if mask_state:
        s = np.zeros_like(s)
    if clip_action:
        a = _clip(a)
    if delta_mask:
        m = np.array([(delta_mask >> c) & 1 for c in range(action_dim)], bool)
        a = a - np.where(m, s, np.float32(0))[:, None, :]
    return np.ascontiguousarray(s, np.float32), np.ascontiguousarray(a, np.float32)


# ------------------------------------------------------------------------------------------------ the estimator from its parts
@dataclasses.dataclass
class ColumnSums:
    """Pass 1 of a key: per column min / max (f32 values) and the f64 sum and sum of squares over `count` rows."""

    count: int
    lo: np.ndarray
    hi: np.ndarray
    sum: np.ndarray
    sumsq: np.ndarray


def check_finite(key: str, sums: ColumnSums) -> None:
    bad = np.flatnonzero(~(np.isfinite(sums.lo) & np.isfinite(sums.hi)))
    if bad.size:
        raise ValueError(f"norm stats: key {key!r}, column {int(bad[0])} holds a non-finite value (min {sums.lo[bad[0]]}, max {sums.hi[bad[0]]});"
                         f" non-finite columns: {bad.tolist()}")  # fmt: skip


def column_edges(lo: float, hi: float, bins: int = QUANTILE_BINS) -> np.ndarray:
    """The edges RunningStats gives a column on its first update."""
    return np.linspace(lo - 1e-10, hi + 1e-10, bins + 1)


def constant_hist(value: float, count: int, edges: np.ndarray) -> np.ndarray:
    """A column with lo == hi never reaches pass 2: its whole count sits in the bin np.histogram names."""
    h, _ = np.histogram(np.array([value], np.float64), bins=edges)
    return h.astype(np.int64) * count


def finish(sums: ColumnSums, hist: np.ndarray, edges: list[np.ndarray]) -> NormStats:
    """mean / std from the sums, q01 / q99 from integer counts: RunningStats.get_statistics on one-shot state."""
    if sums.count < 2:
        raise ValueError("Cannot compute statistics for less than 2 vectors.")
    mean = sums.sum / sums.count
    std = np.sqrt(np.maximum(0, sums.sumsq / sums.count - mean**2))

    def quantile(q):
        return np.array([e[np.searchsorted(np.cumsum(h), q * sums.count)] for h, e in zip(hist, edges, strict=True)])

    return NormStats(mean=mean, std=std, q01=quantile(0.01), q99=quantile(0.99))


def one_shot(rows: np.ndarray) -> NormStats:
    """The defining form: every row at once through the pinned estimator."""
    rs = RunningStats()
    rs.update(np.asarray(rows).astype(np.float64))
    return rs.get_statistics()


# ------------------------------------------------------------------------------------------------ host path (lowered)
def _key_rows(key: str, state, action, ep_end, spec: ChunkSpec, horizon: int, frame_idx, view: dict | None = None) -> np.ndarray:
    s, a = chunk_rows(state, action, ep_end, horizon=horizon if key == "actions" else 1, action_dim=spec.action_dim,
                      clip_state=spec.clip_state, clip_action=spec.clip_action, mask_state=spec.mask_state,
                      delta_mask=spec.delta_mask, frame_idx=frame_idx, **(view or {}))  # fmt: skip
    return (s if key == "state" else a.reshape(-1, spec.action_dim)).astype(np.float64)


def _view_slice(view: dict, sl: slice) -> dict:
    return {k: (v[sl] if k in ("frame_stride", "frame_mirror") and v is not None else v) for k, v in view.items()}


def host_stats(state, action, ep_end, spec: ChunkSpec, horizon: int, frame_idx=None, *, slab_rows: int = HOST_SLAB_ROWS,
               frame_stride=None, frame_mirror=None, left_dim: int = 7, right_dim: int = 7) -> dict[str, NormStats]:  # fmt: skip
    """`chunk_rows` + the one-shot estimator.  A selection that fits one slab goes through RunningStats itself; a larger one takes
    two passes over frame slabs (range and sums, then np.histogram over the fixed edges): the same counts as integers, sums added
    slab by slab.  `frame_stride` / `frame_mirror` (one entry per selected frame) are chunk_rows' view arguments."""
    idx = np.arange(len(state)) if frame_idx is None else np.asarray(frame_idx, np.int64)
    view = {}
    if frame_stride is not None or frame_mirror is not None:
        view = dict(frame_stride=None if frame_stride is None else np.asarray(frame_stride),
                    frame_mirror=None if frame_mirror is None else np.asarray(frame_mirror), left_dim=left_dim, right_dim=right_dim)  # fmt: skip
    out = {}
    for key in KEYS:
        per = max(1, slab_rows // (horizon if key == "actions" else 1))
        if len(idx) <= per:
            x = _key_rows(key, state, action, ep_end, spec, horizon, idx, view)
            check_finite(key, ColumnSums(len(x), x.min(0), x.max(0), None, None))  # np.min / np.max propagate a NaN
            out[key] = one_shot(x)
            continue
        slabs = [slice(i, i + per) for i in range(0, len(idx), per)]
        d = spec.action_dim
        sums = ColumnSums(0, np.full(d, np.inf), np.full(d, -np.inf), np.zeros(d), np.zeros(d))
        for sl in slabs:
            x = _key_rows(key, state, action, ep_end, spec, horizon, idx[sl], _view_slice(view, sl))
            sums.count += len(x)
            sums.lo, sums.hi = np.minimum(sums.lo, x.min(0)), np.maximum(sums.hi, x.max(0))  # (a NaN sticks in both)
            sums.sum += x.sum(0)
            sums.sumsq += (x * x).sum(0)
        check_finite(key, sums)
        edges = [column_edges(sums.lo[c], sums.hi[c]) for c in range(d)]
        hist = np.zeros((d, QUANTILE_BINS), np.int64)
        for sl in slabs:
            x = _key_rows(key, state, action, ep_end, spec, horizon, idx[sl], _view_slice(view, sl))
            for c in range(d):
                hist[c] += np.histogram(x[:, c], bins=edges[c])[0]
        out[key] = finish(sums, hist, edges)
    return out


# ------------------------------------------------------------------------------------------------ device path (lowered)
def _view_args(view) -> tuple | None:
    """(frame_stride pointer, frame_mirror pointer, left_dim, right_dim) of a device view, None for a plain launch.
    `view` = (int32 [M] tensor or None, uint8 [M] tensor or None, left_dim, right_dim)."""
    if view is None:
        return None
    stride, mirror, left_dim, right_dim = view
    return (None if stride is None else stride.data_ptr(), None if mirror is None else mirror.data_ptr(), int(left_dim), int(right_dim))


def device_sums(state, action, ep_end, frame_idx, *, horizon: int, width: int, clip_state: bool, clip_action: bool, mask_state: bool,
                delta_mask: int, view=None) -> ColumnSums:  # fmt: skip
    """kai0_chunk_stats_moments on resident tables (torch tensors on the GPU: f32 [N, ds], f32 [N, da], int32 [N], int32 [M] or None).
    One device-to-host copy of 4 x width doubles.  `view` (see _view_args): kai0_chunk_stats_moments_view instead."""
    import torch

    from . import _lib

    n, m = state.shape[0], (state.shape[0] if frame_idx is None else frame_idx.numel())
    out = torch.empty(4, width, dtype=torch.float64, device=state.device)
    nbytes = _lib.load().kai0_chunk_stats_workspace_bytes(m, width)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=state.device)
    va = _view_args(view)
    _lib.call("kai0_chunk_stats_moments" if va is None else "kai0_chunk_stats_moments_view", state.data_ptr(), state.stride(0),
              min(state.shape[1], width), action.data_ptr(), action.stride(0), action.shape[1], ep_end.data_ptr(), n,
              None if frame_idx is None else frame_idx.data_ptr(), *(va or ()), m, horizon, width,
              int(clip_state), int(clip_action), int(mask_state), delta_mask, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
              torch.cuda.current_stream().cuda_stream)  # fmt: skip
    o = out.cpu().numpy()
    return ColumnSums(count=m * horizon, lo=o[0], hi=o[1], sum=o[2], sumsq=o[3])


def device_hist(state, action, ep_end, frame_idx, edges: np.ndarray, col_mask: int, *, horizon: int, width: int, clip_state: bool,
                clip_action: bool, mask_state: bool, delta_mask: int, view=None) -> np.ndarray:  # fmt: skip
    """kai0_chunk_stats_hist: int64 [width, bins] counts of the columns in col_mask over edges f64 [width, bins + 1] (host array).
    `view` (see _view_args): kai0_chunk_stats_hist_view instead."""
    import torch

    from . import _lib

    bins = edges.shape[1] - 1
    n, m = state.shape[0], (state.shape[0] if frame_idx is None else frame_idx.numel())
    dev_edges = torch.from_numpy(np.ascontiguousarray(edges, np.float64)).to(state.device)
    hist = torch.zeros(width, bins, dtype=torch.int64, device=state.device)
    va = _view_args(view)
    _lib.call("kai0_chunk_stats_hist" if va is None else "kai0_chunk_stats_hist_view", state.data_ptr(), state.stride(0),
              min(state.shape[1], width), action.data_ptr(), action.stride(0), action.shape[1], ep_end.data_ptr(), n,
              None if frame_idx is None else frame_idx.data_ptr(), *(va or ()), m, horizon, width,
              int(clip_state), int(clip_action), int(mask_state), delta_mask, dev_edges.data_ptr(), bins, col_mask, hist.data_ptr(),
              torch.cuda.current_stream().cuda_stream)  # fmt: skip
    return hist.cpu().numpy()


def device_key_stats(key: str, state, action, ep_end, frame_idx, *, bins: int = QUANTILE_BINS, **kw):
    """Both passes of one key and the host-side finishing -> KeyResult.  Columns with
    lo == hi (padding, a masked state, a stuck gripper) never reach pass 2; a non-finite min or max raises ValueError naming the
    key and the column."""
    width = kw["width"]
    # columns past both tables are 0 - 0 whatever the data: the launches take the leading columns that can hold anything else
    live = max(1, min(width, max(action.shape[1], min(state.shape[1], kw["delta_mask"].bit_length()))))
    if kw.get("view") is not None and kw["view"][1] is not None:  # a mirrored frame may move a table column up to left + right - 1
        live = max(live, min(width, kw["view"][2] + kw["view"][3]))
    kw = {**kw, "width": live, "delta_mask": kw["delta_mask"] & ((1 << live) - 1)}
    sums = device_sums(state, action, ep_end, frame_idx, **kw)
    check_finite(key, sums)
    sums = ColumnSums(sums.count, *(np.concatenate([v, np.zeros(width - live)]) for v in (sums.lo, sums.hi, sums.sum, sums.sumsq)))
    edges = np.stack([np.linspace(sums.lo[c] - 1e-10, sums.hi[c] + 1e-10, bins + 1) for c in range(width)])
    varying = [c for c in range(width) if sums.lo[c] != sums.hi[c]]
    col_mask = sum(1 << c for c in varying)
    hist = np.zeros((width, bins), np.int64)
    if col_mask:
        hist[:live] = device_hist(state, action, ep_end, frame_idx, edges[:live], col_mask, **kw)
    for c in range(width):
        if c not in varying:
            hist[c] = constant_hist(sums.lo[c], sums.count, edges[c])
    return KeyResult(sums, hist, edges, finish(sums, hist, list(edges)) if sums.count >= 2 else None)


@dataclasses.dataclass
class KeyResult:
    sums: ColumnSums
    hist: np.ndarray  # int64 [width, bins]
    edges: np.ndarray  # f64 [width, bins + 1]
    stats: NormStats | None  # None for a single row (the estimator refuses it)


def device_stats(state, action, ep_end, spec: ChunkSpec, horizon: int, frame_idx=None, *, device="cuda", **view) -> dict[str, NormStats]:
    res = device_results(state, action, ep_end, spec, horizon, frame_idx, device=device, **view)
    if any(r.stats is None for r in res.values()):
        raise ValueError("Cannot compute statistics for less than 2 vectors.")
    return {key: r.stats for key, r in res.items()}


def device_results(state, action, ep_end, spec: ChunkSpec, horizon: int, frame_idx=None, *, device="cuda", frame_stride=None,
                   frame_mirror=None, left_dim: int = 7, right_dim: int = 7) -> dict[str, KeyResult]:  # fmt: skip
    """The two tables go to the GPU once; two passes per key.  "state" is the horizon = 1, no-delta case of the same kernels with
    the state table in the action slot (a masked state is all zeros: its statistics need no launch).  With `frame_stride` and / or
    `frame_mirror` (host arrays, one entry per frame: a `lerobot_dataset.ViewPlan`) the `_view` entry points run instead; a
    stride whose product with the horizon does not fit int32, or arms that do not fit action_dim, are refused here, before any
    upload or launch."""
    import torch

    state, action = np.ascontiguousarray(state, np.float32), np.ascontiguousarray(action, np.float32)
    n = len(state)
    ep_end = np.asarray(ep_end, np.int64)
    if n >= 2**31 or np.any(ep_end <= np.arange(n)) or np.any(ep_end > n):
        raise ValueError("norm stats: ep_end[i] must lie in (i, N] and N below 2^31")
    if max(state.shape[1], action.shape[1]) > spec.action_dim:
        raise ValueError(f"norm stats: tables of {state.shape[1]} / {action.shape[1]} columns do not fit action_dim = {spec.action_dim}")
    if frame_idx is not None:
        frame_idx = np.asarray(frame_idx, np.int64)
        if frame_idx.size and (frame_idx.min() < 0 or frame_idx.max() >= n):
            raise ValueError("norm stats: frame_idx outside the table")
    m = n if frame_idx is None else len(frame_idx)
    has_view = frame_stride is not None or frame_mirror is not None
    if has_view:
        if left_dim < 0 or right_dim < 0 or left_dim + right_dim > spec.action_dim:
            raise ValueError(f"norm stats: left_dim = {left_dim} + right_dim = {right_dim} do not fit action_dim = {spec.action_dim}")
        for name, v in (("frame_stride", frame_stride), ("frame_mirror", frame_mirror)):
            if v is not None and np.shape(v) != (m,):
                raise ValueError(f"norm stats: {name} must hold one entry per frame ({m}), got shape {np.shape(v)}")
        if frame_stride is not None:
            frame_stride = np.asarray(frame_stride, np.int64)
            if frame_stride.size and (frame_stride.min() < 1 or int(frame_stride.max()) * horizon >= 2**31):
                raise ValueError(f"norm stats: frame_stride must lie in [1, 2^31 / horizon), got {frame_stride.min()}..{frame_stride.max()}")
    dev = torch.device(device)
    t_state, t_action = torch.from_numpy(state).to(dev), torch.from_numpy(action).to(dev)
    t_end = torch.from_numpy(ep_end.astype(np.int32)).to(dev)
    t_idx = None if frame_idx is None else torch.from_numpy(frame_idx.astype(np.int32)).to(dev)
    view = None
    if has_view:
        view = (None if frame_stride is None else torch.from_numpy(frame_stride.astype(np.int32)).to(dev),
                None if frame_mirror is None else torch.from_numpy(np.ascontiguousarray(np.asarray(frame_mirror) != 0, np.uint8)).to(dev),
                left_dim, right_dim)  # fmt: skip
    d = spec.action_dim
    out = {}
    with torch.cuda.device(dev):
        if spec.mask_state:
            zeros = ColumnSums(m, np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d))
            edges = np.stack([column_edges(0.0, 0.0) for _ in range(d)])
            hist = np.stack([constant_hist(0.0, m, e) for e in edges])
            out["state"] = KeyResult(zeros, hist, edges, finish(zeros, hist, list(edges)) if m >= 2 else None)
        else:
            out["state"] = device_key_stats("state", t_state, t_state, t_end, t_idx, horizon=1, width=d, clip_state=False,
                                            clip_action=spec.clip_state, mask_state=False, delta_mask=0, view=view)  # fmt: skip
        out["actions"] = device_key_stats("actions", t_state, t_action, t_end, t_idx, horizon=horizon, width=d,
                                          clip_state=spec.clip_state, clip_action=spec.clip_action, mask_state=spec.mask_state,
                                          delta_mask=spec.delta_mask, view=view)  # fmt: skip
    return out


# ------------------------------------------------------------------------------------------------ loader path (not lowered)
def loader_stats(config, data_config, frame_idx=None) -> dict[str, NormStats]:
    """compute_norm_stats.py:24-57,102-109: the dataset through `repack_transforms.inputs + data_transforms.inputs`, batches of
    `config.batch_size` samples through RunningStats (every selected frame: the last, shorter batch included)."""
    from . import lerobot_dataset as lrd
    from .data_loader import TransformedDataset

    dataset = lrd.create_torch_dataset(data_config, config.model.action_horizon, config.model)
    dataset = TransformedDataset(dataset, [*data_config.repack_transforms.inputs, *data_config.data_transforms.inputs])
    idx = np.arange(len(dataset)) if frame_idx is None else np.asarray(frame_idx)
    stats = {key: RunningStats() for key in KEYS}
    for i in range(0, len(idx), config.batch_size):
        samples = [dataset[int(j)] for j in idx[i : i + config.batch_size]]
        for key in KEYS:
            stats[key].update(np.stack([np.asarray(s[key]) for s in samples]))
    return {key: s.get_statistics() for key, s in stats.items()}


# ------------------------------------------------------------------------------------------------ public interface
def _sample(n: int, max_frames: int | None, seed: int):
    if max_frames is None or max_frames >= n:
        return None
    return np.sort(np.random.default_rng(seed).choice(n, size=max_frames, replace=False))


def _config_plan(data_config, meta, episodes, state, action, ep_end):
    """The ViewPlan `create_torch_dataset` gives this data config, from the episode boundaries of the tables alone."""
    from . import lerobot_dataset as lrd

    eps = list(episodes) if episodes is not None else sorted(meta.episodes)
    ends, lengths = np.unique(ep_end, return_counts=True)
    if len(lengths) != len(eps):
        raise ValueError(f"{meta.root}: {len(eps) - len(lengths)} of the selected episodes hold no frame")
    if data_config.space_mirror:
        total = data_config.left_dim + data_config.right_dim
        if state.shape[1] != total or action.shape[1] != total:  # swap_arms_in_array's error, before anything is computed
            raise ValueError(f"Array dimension mismatch: expected {total} dims (left{data_config.left_dim} + right{data_config.right_dim}), "
                             f"got {state.shape[1]} / {action.shape[1]} dims")  # fmt: skip
    return lrd.plan_view(lengths, eps, data_config.time_scaling, data_config.space_mirror)


def compute_norm_stats(config, *, max_frames: int | None = None, seed: int = 0, device=None) -> dict[str, NormStats]:
    """{"state": NormStats, "actions": NormStats} of a TrainConfig's dataset (`config`: the TrainConfig or its name).
    Lowered transform stack + a GPU: the two columns are read from the parquet files and reduced by the HIP kernels.  Otherwise the
    host: `chunk_rows` + the one-shot estimator where the stack lowers, the reference's loop over the transformed dataset where it
    does not.  `max_frames`: a seeded sample of frames without replacement.  `device="cpu"` forces the host."""
    import torch

    from . import lerobot_dataset as lrd
    from .training_config import get_config

    if isinstance(config, str):
        config = get_config(config)
    data_config = config.data.create(config.assets_dirs, config.model)
    if data_config.repo_id is None or data_config.repo_id == "fake":
        raise ValueError("Data config must have a repo_id naming a LeRobot dataset directory")
    spec = lower_transforms(data_config)
    why = None if spec is not None else "its input transforms hold more than repack / AgilexInputs / DeltaActions"
    meta = lrd.LeRobotDatasetMetadata(data_config.repo_id)
    if spec is not None:
        feats = [meta.features.get(c, {}) for c in (spec.state_col, spec.action_col)]
        if any(f.get("dtype") != "float32" for f in feats):
            spec, why = None, "the state / action columns are not float32 features"
        elif any(int(np.prod(f.get("shape", [0]))) > spec.action_dim for f in feats):
            spec, why = None, f"the state / action columns are wider than action_dim = {spec.action_dim}"
    episodes = data_config.episodes
    if getattr(config, "advantage_estimator", False):  # create_advantage_torch_dataset's episode selection
        episodes = lrd.episodes_split_through_task(data_config.repo_id, split_type=getattr(config, "split", "all") or "all")
        data_config = dataclasses.replace(data_config, episodes=episodes)
    if spec is None:
        logger.info("norm stats of %s on the host, through the transformed dataset: %s", data_config.repo_id, why)
        eps = list(episodes) if episodes is not None else sorted(meta.episodes)
        n = len(lrd.plan_view([meta.episodes[e]["length"] for e in eps], eps, data_config.time_scaling, data_config.space_mirror))
        return loader_stats(config, data_config, _sample(n, max_frames, seed))
    state, action, ep_end = lrd.read_state_action_columns(data_config.repo_id, spec.state_col, spec.action_col, episodes=episodes)
    view = {}
    if data_config.space_mirror or data_config.time_scaling is not None:
        # the statistics of the AUGMENTED dataset: every sample the loader will yield, as (row, stride, mirrored)
        plan = _config_plan(data_config, meta, episodes, state, action, ep_end)
        pick = _sample(len(plan), max_frames, seed)
        pick = slice(None) if pick is None else pick
        frame_idx = plan.frame_idx[pick]
        view = dict(frame_stride=plan.frame_stride[pick], frame_mirror=plan.frame_mirror[pick], left_dim=data_config.left_dim,
                    right_dim=data_config.right_dim)  # fmt: skip
    else:
        frame_idx = _sample(len(state), max_frames, seed)
    horizon = config.model.action_horizon
    use_gpu = torch.cuda.is_available() if device is None else torch.device(device).type == "cuda"
    if not use_gpu:
        logger.info("norm stats of %s on the host (%s): chunk_rows + the one-shot estimator", data_config.repo_id,
                    "device='cpu' was asked for" if device is not None else "no GPU is present")  # fmt: skip
        return host_stats(state, action, ep_end, spec, horizon, frame_idx, **view)
    return device_stats(state, action, ep_end, spec, horizon, frame_idx, device=device or "cuda", **view)


def output_dir(config) -> pathlib.Path:
    """Where `DataConfigFactory._load_norm_stats` looks: assets_dir / asset_id (asset_id defaults to the repo_id)."""
    data_config = config.data.create(config.assets_dirs, config.model)
    return pathlib.Path(config.data.assets.assets_dir or config.assets_dirs) / (data_config.asset_id or data_config.repo_id)


def save(config, norm_stats: dict[str, NormStats]) -> pathlib.Path:
    out = output_dir(config)
    _normalize.save(out, norm_stats)
    return out / "norm_stats.json"
