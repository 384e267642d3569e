"""Stage-Advantage annotation, host side (kai0_amd/stage_advantage.py): the frame-preprocessing restatement calibrated against
torch, the executed-reference golden of the evaluator and of discretize_advantage.py, `plan_episode`'s properties, and a parquet round
trip of `annotate_dataset` / `discretize` through the CLI.  No GPU."""

import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import stage_advantage_refs as refs  # noqa: E402

from kai0_amd import stage_advantage as sa  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "stage_advantage.npz")
SHAPES = [(480, 640, 224), (640, 480, 224), (225, 223, 224), (37, 53, 224), (30, 40, 56), (224, 224, 224)]


# ------------------------------------------------------------------------------------------------ 1. the frame restatement
@pytest.mark.parametrize("h0,w0,size", SHAPES)
def test_frame_restatement_matches_resize_with_pad_torch(h0, w0, size):
    """`frames_to_chw_ref` (the f32 restatement the GPU kernel is held to) vs `resize_with_pad_torch` on the evaluator's normalised
    input, noise images.  Bound 1e-4: a restatement with an unfused source index differs from torch by up to 1.5e-5 at these shapes
    (ceiling 8 * 2^-23 * max(H0, W0) = 6e-4 at 640), while a wrong half-pixel or pad convention shows as >= 1e-2 on noise.  With
    the contractions of torch's CPU kernel written out (stage_advantage_refs) the restatement is bit-identical to torch where torch
    does not split the image over threads (one thread, or an output below its parallel grain such as 56 x 56) and within 1.8e-7 of
    its multi-threaded form (measured, 224 x 224 outputs at 8 threads)."""
    rng = np.random.default_rng(h0 * 1000 + w0)
    frames = rng.integers(0, 256, size=(2, h0, w0, 3), dtype=np.uint8)
    got = refs.frames_to_chw_ref(frames, size, size)
    want = torch.stack([refs.evaluator_image(f, size, size) for f in frames]).numpy()
    assert got.shape == want.shape == (2, 3, size, size) and got.dtype == np.float32
    d = float(np.abs(got - want).max())
    print(f"restatement vs resize_with_pad_torch {h0}x{w0} -> {size}: max|d| = {d:.3e}")
    assert d <= 1e-4
    rh, rw, ph0, pw0 = refs.resize_geometry(h0, w0, size, size)
    pad = np.ones((size, size), dtype=bool)
    pad[ph0 : ph0 + rh, pw0 : pw0 + rw] = False
    assert (got[:, :, pad] == -1.0).all() and (want[:, :, pad] == -1.0).all()
    if (h0, w0) == (size, size):
        assert np.array_equal(got, want)  # no resize: the normalisation alone, exact
    assert refs.resize_geometry(h0, w0, size, size) == __import__("kai0_amd.ops", fromlist=["x"]).resize_geometry(h0, w0, size, size)


# ------------------------------------------------------------------------------------------------ 2. executed-reference golden
def _episode_values(G, two_timesteps: bool):
    """The observations of the golden's episode rebuilt from `plan_episode`'s slot tables and the restatement, through the stub model."""
    frames = G["frames"]  # [3, F, H0, W0, 3]
    F, interval, bs = frames.shape[1], int(G["relative_interval"]), int(G["batch_size"])
    images = np.stack([refs.frames_to_chw_ref(frames[c], 224, 224) for c in range(3)], axis=1)  # [F, cam, 3, 224, 224]
    ring = np.zeros((sa.ring_size(interval, bs), 3, 3, 224, 224), dtype=np.float32)
    raw = np.zeros((2, F), dtype=np.float32)
    seen = []
    for plan in sa.plan_episode(F, interval, bs, two_timesteps):
        for f in range(*plan.fill):
            ring[sa.ring_slot(f, interval, bs)] = images[f]
        seen += plan.frames
        for p, table in ((0, plan.relative_slots), (1, plan.absolute_slots)):
            if table is None:
                continue
            stack = np.stack([np.concatenate([ring[s] for s in row]) for row in table])  # [B, nslot, 3, 224, 224], (timestep, camera)
            raw[p, list(plan.frames)] = refs.stub_values_from_stack(stack)
    assert seen == list(range(F))
    return raw


@pytest.mark.parametrize("mode", ["two", "one"])
def test_evaluator_golden(mode):
    """The reference's evaluate_video_2timesteps_advantages / evaluate_video_1timestep_advantage, executed from its own source on
    seeded frames with a stub model (tests/golden/make_stage_advantage_golden.py), vs plan_episode + the restatement + the same stub +
    advantages_from_values: every field to 1e-6, the indices exactly.  relative_interval = 3, batch_size = 4 over 9 frames: frames with
    the full interval, clamped futures (rescaled by interval / gap) and the last frame (future == frame: zeros)."""
    G = np.load(GOLDEN)
    two = mode == "two"
    raw = _episode_values(G, two)
    out = sa.advantages_from_values(raw[1], raw[0] if two else None, relative_interval=int(G["relative_interval"]))
    fields = [k[len(mode) + 1 :] for k in G.files if k.startswith(mode + ".")]
    assert set(fields) == set(out) and ("relative_advantage" in fields) == two
    for k in fields:
        want = G[f"{mode}.{k}"]
        if k.endswith("_idx"):
            assert np.array_equal(out[k], want), k
        else:
            d = float(np.abs(out[k] - want).max())
            print(f"{mode}.{k}: max|d| = {d:.3e}")
            assert d <= 1e-6, (k, d)
    gap = G[f"{mode}.future_frame_idx"] - G[f"{mode}.frame_idx"]
    assert (gap == 3).any() and ((gap > 0) & (gap < 3)).any() and (gap == 0).sum() == 1  # every branch of the post-processing
    assert np.abs(G[f"{mode}.absolute_value"][1:]).min() > 1e-3  # the stub's values are not degenerate


def _write_table(root, G):
    import pandas as pd

    os.makedirs(root / "data" / "chunk-000")
    lo = 0
    for i, n in enumerate(G["disc.lengths"]):
        cols = {k: G[f"disc.{k}"][lo : lo + n] for k in ("absolute_advantage", "relative_advantage", "stage_progress_gt")}
        pd.DataFrame({"frame_index": np.arange(n), **cols}).to_parquet(root / "data" / "chunk-000" / f"episode_{i:06d}.parquet")
        lo += n


@pytest.mark.parametrize("case", ["binary", "binary_rel_staged2", "slices5", "slices4_staged3"])
def test_discretize_golden(case, tmp_path):
    """discretize_advantage.py's `main`, executed from the reference's source on a two-episode table, vs the CLI of this module with
    the same arguments: the `task_index` column of every frame and tasks.jsonl, exactly."""
    import pandas as pd

    G = np.load(GOLDEN)
    _write_table(tmp_path, G)
    assert sa.main(["discretize", str(tmp_path), *[str(a) for a in G[f"disc.{case}.argv"]]]) == 0
    files = sorted((tmp_path / "data" / "chunk-000").glob("*.parquet"))
    got = np.concatenate([pd.read_parquet(f)["task_index"].values for f in files])
    assert got.dtype == np.int32 and np.array_equal(got, G[f"disc.{case}.task_index"])
    tasks = [json.loads(line) for line in open(tmp_path / "meta" / "tasks.jsonl")]
    assert [t["task"] for t in tasks] == list(G[f"disc.{case}.tasks"]) and [t["task_index"] for t in tasks] == list(range(len(tasks)))
    assert len(set(got.tolist())) > 1


def test_discretize_pieces_golden(tmp_path):
    """get_stage_index over the table (1.0 joins the last stage, 0.5 opens the second of two), and --dry-run writes nothing."""
    G = np.load(GOLDEN)
    assert [sa.get_stage_index(s, 3) for s in G["disc.stage_progress_gt"]] == list(G["disc.stage_index_3"])
    assert sa.get_stage_index(1.0, 2) == 1 and sa.get_stage_index(0.5, 2) == 1 and sa.get_stage_index(0.49, 2) == 0 and sa.get_stage_index(0.7, 1) == 0
    _write_table(tmp_path, G)
    before = {f: f.read_bytes() for f in (tmp_path / "data" / "chunk-000").glob("*.parquet")}
    res = sa.discretize(tmp_path, threshold=30, dry_run=True)
    assert not (tmp_path / "meta").exists() and all(f.read_bytes() == b for f, b in before.items())
    adv = G["disc.absolute_advantage"].astype(np.float32)
    assert res["frames"] == {0: 40} and res["thresholds"][0] == np.percentile(adv.tolist(), 70)
    with pytest.raises(ValueError):
        sa.discretize(tmp_path / "nowhere")
    with pytest.raises(ValueError):
        sa.discretize(tmp_path, advantage_source="progress")


# ------------------------------------------------------------------------------------------------ 3. plan_episode
@pytest.mark.parametrize("F,interval,bs", [(9, 3, 2), (9, 3, 4), (2, 50, 16), (40, 50, 16), (51, 50, 16), (137, 50, 16), (23, 5, 7), (64, 50, 8)])
@pytest.mark.parametrize("two", [True, False])
def test_plan_episode_properties(F, interval, bs, two):
    """Every frame once and in order; futures = min(n + interval, F - 1); the fills are ascending, disjoint and cover exactly what the
    batches read; slot tables stay inside a ring of interval + batch_size + 1; and — replaying the fills — every slot a batch reads
    holds the frame the batch means (nothing is overwritten while still needed)."""
    plans = sa.plan_episode(F, interval, bs, two)
    assert [f for p in plans for f in p.frames] == list(range(F))
    ring = sa.ring_size(interval, bs)
    assert ring == interval + bs + 1
    held, filled = {}, 0
    for p in plans:
        assert 1 <= len(p.frames) <= bs and p.futures == tuple(min(n + interval, F - 1) for n in p.frames)
        assert p.fill[0] == filled and p.fill[1] >= filled
        for f in range(*p.fill):
            held[sa.ring_slot(f, interval, bs)] = f
        filled = p.fill[1]
        if two:
            assert [held[a] for a, _ in p.relative_slots] == list(p.frames) and [held[b] for _, b in p.relative_slots] == list(p.futures)
            assert [held[a] for a, _ in p.absolute_slots] == [0] * len(p.frames) and [held[b] for _, b in p.absolute_slots] == list(p.frames)
        else:
            assert p.relative_slots is None and [held[a] for (a,) in p.absolute_slots] == list(p.frames)
        tables = (p.relative_slots or ()) + p.absolute_slots
        assert all(0 <= s < ring for row in tables for s in row)
    assert filled == F  # each frame encoded exactly once


def test_plan_episode_and_advantages_refuse_short_episodes():
    for n in (0, 1):
        with pytest.raises(ValueError):
            sa.plan_episode(n, 3, 2)
        with pytest.raises(ValueError):
            sa.advantages_from_values(np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), relative_interval=3)
    out = sa.advantages_from_values(np.float32([0.9, 0.5]), np.float32([0.4, 0.7]), relative_interval=50)  # F = 2 <= interval
    assert out["future_frame_idx"].tolist() == [1, 1] and out["absolute_value"].tolist() == [0.0, float(np.float32(0.5))]
    assert out["relative_advantage"].tolist() == [1.0, 0.0]  # 0.4 / 1 * 50 clamps to 1; the last frame is 0
    assert out["absolute_advantage"].tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ 4. parquet round trip
class _StubAnnotator:
    """Stands in for ValueAnnotator (which needs a GPU): values from the frames' means, through the real post-processing."""

    def __init__(self):
        self.calls = []

    def annotate(self, frames, tokens, token_mask, *, two_timesteps=True, relative_interval=50, **kw):
        self.calls.append((frames[0].shape[0], two_timesteps, relative_interval))
        means = np.stack([f.reshape(f.shape[0], -1).mean(axis=1) for f in frames]).mean(axis=0)
        absolute = np.tanh((means - 100.0) / 50.0).astype(np.float32)
        return sa.advantages_from_values(absolute, (absolute * 0.5).astype(np.float32) if two_timesteps else None,
                                         relative_interval=relative_interval)  # fmt: skip


def _make_dataset(root, lengths=(7, 5)):
    import pandas as pd

    (root / "meta").mkdir(parents=True)
    info = {"fps": 30, "chunks_size": 1000, "total_episodes": len(lengths),
            "data_path": "data/chunk-{episode_chunk:03d}/episode_{episode_index:06d}.parquet",
            "video_path": "videos/chunk-{episode_chunk:03d}/{video_key}/episode_{episode_index:06d}.mp4",
            "features": {f"observation.images.{k}": {"dtype": "video"} for k in sa.CAMERA_KEYS}}  # fmt: skip
    (root / "meta" / "info.json").write_text(json.dumps(info))
    (root / "meta" / "tasks.jsonl").write_text(json.dumps({"task_index": 0, "task": "fold the cloth"}) + "\n")
    (root / "meta" / "episodes.jsonl").write_text("".join(json.dumps({"episode_index": i, "length": n}) + "\n" for i, n in enumerate(lengths)))
    for i, n in enumerate(lengths):
        (root / "data" / "chunk-000").mkdir(parents=True, exist_ok=True)
        pd.DataFrame({"frame_index": np.arange(n), "episode_index": np.full(n, i), "task_index": np.zeros(n, dtype=np.int64),
                      "stage_progress_gt": np.linspace(0, 1, n)}).to_parquet(root / "data" / "chunk-000" / f"episode_{i:06d}.parquet")  # fmt: skip
        for k in sa.CAMERA_KEYS:
            d = root / "videos" / "chunk-000" / f"observation.images.{k}"
            d.mkdir(parents=True, exist_ok=True)
            (d / f"episode_{i:06d}.mp4").write_bytes(b"")  # decoded by the test's frame_decoder


def _decoder(path, timestamps, tolerance_s):
    ep = int(str(path)[-10:-4])
    cam = [k in str(path) for k in sa.CAMERA_KEYS].index(True)
    rng = np.random.default_rng(100 * ep + cam)
    video = rng.integers(0, 256, size=(64, 6, 8, 3), dtype=np.uint8)
    return video[[round(t * 30) for t in timestamps]]


def test_annotate_dataset_and_discretize_round_trip(tmp_path, monkeypatch):
    """eval.py's loop then discretize_advantage.py on a two-episode temporary dataset, end to end through the CLI: the estimator is a
    stub (`load_annotator` needs a GPU) and the videos come from lerobot_dataset's decoder plug."""
    import pandas as pd
    import pyarrow.parquet as pq

    from kai0_amd import lerobot_dataset as lrd

    root = tmp_path / "ds"
    _make_dataset(root)
    stub = _StubAnnotator()
    monkeypatch.setattr(sa, "load_annotator", lambda *a, **k: (stub, np.arange(8), np.arange(8) < 5))
    monkeypatch.setattr(lrd, "_default_frame_decoder", _decoder)
    assert sa.main(["annotate", str(root), "--ckpt", "unused", "--steps", "123", "--relative-interval", "3", "--shard", "1/2"]) == 0
    out_dir = root / "data_KAI0_123" / "chunk-000"
    assert sorted(p.name for p in out_dir.iterdir()) == ["episode_000001.parquet"] and stub.calls == [(5, True, 3)]  # shard 1 of 2
    assert sa.main(["annotate", str(root), "--ckpt", "unused", "--steps", "123", "--relative-interval", "3"]) == 0
    assert stub.calls == [(5, True, 3), (7, True, 3)]  # the existing output was skipped
    for ep, n in enumerate((7, 5)):
        src = pq.read_table(root / "data" / "chunk-000" / f"episode_{ep:06d}.parquet")
        got = pq.read_table(out_dir / f"episode_{ep:06d}.parquet")
        assert got.column_names == src.column_names + list(sa.ADVANTAGE_COLUMNS) and got.num_rows == n
        assert got.select(src.column_names).equals(src)
        frames = [_decoder(root / "videos" / "chunk-000" / f"observation.images.{k}" / f"episode_{ep:06d}.mp4", [i / 30 for i in range(n)], 0)
                  for k in sa.CAMERA_KEYS]  # fmt: skip
        want = _StubAnnotator().annotate(frames, None, None, relative_interval=3)
        for k in sa.ADVANTAGE_COLUMNS:
            assert np.array_equal(np.asarray(got[k].to_pylist()), want[k]), k
        assert got["absolute_value"][0].as_py() == 0.0 and got["relative_advantage"][n - 1].as_py() == 0.0
    # one-timestep mode: no relative_advantage column
    assert sa.main(["annotate", str(root), "--ckpt", "unused", "--one-timestep", "--relative-interval", "3", "--shard", "0/2"]) == 0
    one = pq.read_table(root / "data_PI06_100000" / "chunk-000" / "episode_000000.parquet")
    assert "relative_advantage" not in one.column_names and "absolute_advantage" in one.column_names
    # step 2b: discretise the annotated copy in place
    ann = tmp_path / "annotated"
    (ann / "data").mkdir(parents=True)
    os.rename(root / "data_KAI0_123" / "chunk-000", ann / "data" / "chunk-000")
    assert sa.main(["discretize", str(ann), "--threshold", "30", "--stage-nums", "2"]) == 0
    labels = np.concatenate([pd.read_parquet(f)["task_index"].values for f in sorted((ann / "data" / "chunk-000").glob("*.parquet"))])
    assert set(labels.tolist()) == {0, 1} and len(labels) == 12
    assert [json.loads(line)["task"] for line in open(ann / "meta" / "tasks.jsonl")] == [
        "fold the cloth, Advantage: negative", "fold the cloth, Advantage: positive"]  # fmt: skip
    with pytest.raises(ValueError):
        sa.parse_shard("2/2")


def test_video_decoding_unavailable_is_a_clear_error(tmp_path, monkeypatch):
    """Neither PyAV nor OpenCV importable: annotate_dataset surfaces lerobot_dataset's VideoDecodeUnavailable, naming the remedy."""
    from kai0_amd import lerobot_dataset as lrd

    monkeypatch.setitem(sys.modules, "av", None)  # `import av` / `import cv2` raise ImportError
    monkeypatch.setitem(sys.modules, "cv2", None)
    root = tmp_path / "ds"
    _make_dataset(root, lengths=(3,))
    with pytest.raises(lrd.VideoDecodeUnavailable, match="frame_decoder"):
        sa.annotate_dataset(_StubAnnotator(), root, np.arange(8), np.arange(8) < 5, name="KAI0", steps=1)


def test_prototypes_and_bindings():
    """The two prototypes are in include/kai0hip.h, cite the reference op they replace, and _lib.py binds them; the C ABI version is 3."""
    import ctypes as C

    from kai0_amd import _lib
    from kai0_amd.build import SRC

    header = open(os.path.join(os.path.dirname(HERE), "include", "kai0hip.h")).read()
    assert "int kai0_frames_to_chw(const uint8_t* frames, float* out, int N, int H0, int W0, int H, int W, int rh, int rw, int ph0, int pw0," in header
    assert "int kai0_prefix_gather(const void* bank, const int32_t* slots, const void* lang, void* out, int B, int nslot, int n_img, int T, int D," in header
    assert "evaluator.py:151-165" in header and "pi0_pytorch.py:186-235" in header
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert _lib._PROTOS["kai0_frames_to_chw"] == [p, p, i, i, i, i, i, i, i, i, i, p]
    assert _lib._PROTOS["kai0_prefix_gather"] == [p, p, p, p, i, i, i, i, i, i64, p]
    assert "frames.hip" in SRC and _lib.ABI_VERSION == 4
