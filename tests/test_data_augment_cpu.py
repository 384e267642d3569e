"""Train-deploy alignment as dataset views (kai0_amd.lerobot_dataset: MirroredView / with_mirror / TimeScaling / view_plan;
normalize.mirror_norm_stats).

Space mirroring is held to the reference's own functions through tests/golden/data_augment.{npz,json}
(tests/golden/make_data_augment_golden.py executes them).  The time-scaling arithmetic sits inside reference functions that import
`lerobot`, so it is pinned by literal cases worked out from the cited lines of time_scaling.py: new_ep_length = (L + N - 1) // N (:207),
kept rows range(0, L, N) (:256), frame_index = 0..L'-1 and timestamp = j / fps (:274-297), and lerobot's window clamp on the
shortened episode.  Everything runs on a synthetic image-LeRobot directory: episodes of 7, 10 and 1 frames, three cameras of 8 x 6
pixels whose every pixel column differs, 14-value state and action rows whose every column differs."""

import dataclasses
import io
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from kai0_amd import lerobot_dataset as lrd  # noqa: E402
from kai0_amd import norm_stats as ns  # noqa: E402
from kai0_amd import normalize  # noqa: E402
from kai0_amd import training_config as tc  # noqa: E402
from kai0_amd.data_loader import TransformedDataset  # noqa: E402

FPS = 30
LENGTHS = [7, 10, 1]
STARTS = [0, 7, 17]
CAMS = ("top_head", "hand_left", "hand_right")
HORIZON = 5
IMG_H, IMG_W = 6, 8
GOLD_NPZ = np.load(os.path.join(HERE, "golden", "data_augment.npz"))
GOLD = json.load(open(os.path.join(HERE, "golden", "data_augment.json")))


def _tok():
    return np.load(os.path.join(HERE, "golden", "host_pipeline.npz"))["tok.model"].tobytes()


def _image(ep: int, fr: int, cam: int) -> np.ndarray:
    img = np.zeros((IMG_H, IMG_W, 3), np.uint8)
    img[..., 0], img[..., 1] = 10 * ep + 40 * cam + 1, 5 * fr + 2
    img[..., 2] = np.arange(IMG_W) * 20 + np.where(np.arange(IMG_W) < IMG_W // 2, 3, 90)  # the two halves, and every column, differ
    return img


def _png(arr: np.ndarray) -> bytes:
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def _state(ep: int, fr: int) -> np.ndarray:
    return ((100 * ep + fr) / 1000 + np.arange(14) * 0.1 - 0.6).astype(np.float32)


def _action(ep: int, fr: int) -> np.ndarray:
    return ((100 * ep + fr) / 100 + np.arange(14) * 0.01 - 1.0).astype(np.float32)


def make_dataset(root):
    import pyarrow as pa
    import pyarrow.parquet as pq

    (root / "meta").mkdir(parents=True)
    feats = {"observation.state": {"dtype": "float32", "shape": [14]}, "action": {"dtype": "float32", "shape": [14]},
             "timestamp": {"dtype": "float32", "shape": [1]}, "frame_index": {"dtype": "int64", "shape": [1]},
             "episode_index": {"dtype": "int64", "shape": [1]}, "index": {"dtype": "int64", "shape": [1]},
             "task_index": {"dtype": "int64", "shape": [1]}, "stage_progress_gt": {"dtype": "float32", "shape": [1]},
             "progress_gt": {"dtype": "float32", "shape": [1]},
             **{f"observation.images.{cam}": {"dtype": "image", "shape": [IMG_H, IMG_W, 3]} for cam in CAMS}}  # fmt: skip
    info = {"codebase_version": "v2.1", "fps": FPS, "chunks_size": 1000, "total_episodes": len(LENGTHS), "features": feats,
            "data_path": "data/chunk-{episode_chunk:03d}/episode_{episode_index:06d}.parquet",
            "video_path": "videos/chunk-{episode_chunk:03d}/{video_key}/episode_{episode_index:06d}.mp4"}  # fmt: skip
    (root / "meta" / "info.json").write_text(json.dumps(info))
    (root / "meta" / "tasks.jsonl").write_text(json.dumps({"task_index": 0, "task": "Flatten and fold the cloth."}))
    (root / "meta" / "episodes.jsonl").write_text(
        "\n".join(json.dumps({"episode_index": e, "tasks": ["Flatten and fold the cloth."], "length": n}) for e, n in enumerate(LENGTHS)))
    g = 0
    for e, n in enumerate(LENGTHS):
        arrays = {"observation.state": pa.array([list(_state(e, f)) for f in range(n)], type=pa.list_(pa.float32())),
                  "action": pa.array([list(_action(e, f)) for f in range(n)], type=pa.list_(pa.float32())),
                  "timestamp": pa.array(np.arange(n, dtype=np.float32) / FPS), "frame_index": pa.array(np.arange(n)),
                  "episode_index": pa.array(np.full(n, e)), "index": pa.array(np.arange(g, g + n)),
                  "task_index": pa.array(np.zeros(n, np.int64)),
                  "stage_progress_gt": pa.array(((np.arange(n) + 1) / (n + 1)).astype(np.float32)),
                  "progress_gt": pa.array(((np.arange(n) + 1) / (n + 1)).astype(np.float32)),
                  **{f"observation.images.{cam}": pa.array([{"bytes": _png(_image(e, f, c)), "path": None} for f in range(n)])
                     for c, cam in enumerate(CAMS)}}  # fmt: skip
        p = root / f"data/chunk-000/episode_{e:06d}.parquet"
        p.parent.mkdir(parents=True, exist_ok=True)
        pq.write_table(pa.table(arrays), p)
        g += n
    return root


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return make_dataset(tmp_path_factory.mktemp("augment") / "FlattenFold")


def _windows(root, **kw):
    return lrd.LeRobotDataset(root, delta_timestamps={"action": [t / FPS for t in range(HORIZON)]}, **kw)


def _pixels(img: torch.Tensor) -> np.ndarray:
    return (img * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()


def _same(a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (set(a) ^ set(b))
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (str, int, float, bool)) or a is None:
        assert a == b
    else:
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def _hand_mirror(item: dict, prefixes=("",)) -> dict:
    """What space_mirroring.py leaves of a raw sample, written out by hand: arms swapped, every camera flipped, hand cameras traded."""
    out = dict(item)
    for p in prefixes:
        for key in ("observation.state", "action"):
            v = item[p + key]
            out[p + key] = torch.cat([v[..., 7:], v[..., :7]], dim=-1)
        cam = p + "observation.images."
        out[cam + "top_head"] = torch.flip(item[cam + "top_head"], dims=[-1])
        out[cam + "hand_left"] = torch.flip(item[cam + "hand_right"], dims=[-1])
        out[cam + "hand_right"] = torch.flip(item[cam + "hand_left"], dims=[-1])
    return out


# ------------------------------------------------------------------------------------------------ space mirroring: the fixture
def test_rows_and_norm_stats_against_the_reference():
    rows = GOLD_NPZ["rows"]
    assert np.array_equal(normalize.swap_arms(rows), GOLD_NPZ["rows_swapped_7_7"])  # a whole [T, 14] window at once
    assert np.array_equal(normalize.swap_arms(rows, 6, 8), GOLD_NPZ["rows_swapped_6_8"])
    for r, want in zip(rows, GOLD_NPZ["rows_swapped_7_7"], strict=True):
        assert np.array_equal(normalize.swap_arms(r), want)
        assert torch.equal(normalize.swap_arms(torch.from_numpy(r)), torch.from_numpy(want))
    assert not np.array_equal(GOLD_NPZ["rows_swapped_7_7"], -rows[:, ::-1])  # a swap: no sign change, no reversal
    with pytest.raises(ValueError) as e:
        normalize.swap_arms(np.zeros(16, np.float32))
    assert str(e.value) == GOLD["wrong_length_error"]
    # lists with padding: the entries after the arms stay
    for name, dims in (("list14_swapped", (7, 7)), ("list32_swapped", (7, 7)), ("list32_swapped_5_9", (5, 9))):
        src = np.array(GOLD[name.split("_swapped")[0]])
        assert np.array_equal(src[normalize.arm_swap_perm(len(src), *dims)], np.array(GOLD[name])), name
    assert GOLD["list32_swapped"][14:] == GOLD["list32"][14:]
    with pytest.raises(ValueError) as e:
        normalize.arm_swap_perm(10)
    assert str(e.value) == GOLD["short_list_error"]
    # a whole norm_stats.json
    stats = normalize.deserialize_json(json.dumps(GOLD["norm_stats_in"]))
    want = normalize.deserialize_json(json.dumps(GOLD["norm_stats_out"]))
    got = normalize.mirror_norm_stats(stats)
    assert set(got) == {"state", "actions", "extra"}
    for key in got:
        for f in ("mean", "std", "q01", "q99"):
            a, b = getattr(got[key], f), getattr(want[key], f)
            assert (a is None and b is None) or np.array_equal(a, b), (key, f)
    assert np.array_equal(got["state"].mean[14:], stats["state"].mean[14:]) and not np.array_equal(got["state"].mean[:14], stats["state"].mean[:14])
    assert np.array_equal(got["extra"].mean, stats["extra"].mean)  # keys other than state / actions are left alone
    back = normalize.mirror_norm_stats(got)
    for key in back:
        for f in ("mean", "std", "q01", "q99"):
            a, b = getattr(back[key], f), getattr(stats[key], f)
            assert (a is None and b is None) or np.array_equal(a, b), (key, f)
    with pytest.raises(ValueError, match="Insufficient array dimensions"):
        normalize.mirror_norm_stats({"state": normalize.NormStats(mean=np.zeros(10), std=np.ones(10))})
    # the per-episode statistics of the fixture: the hand cameras trade places (what camera_mirror_map encodes)
    cams = [f"observation.images.{c}" for c in CAMS]
    for cam, src in lrd.camera_mirror_map(cams).items():
        assert GOLD["episode_stats_out"][cam] == GOLD["episode_stats_in"][src]
    assert np.array_equal(normalize.swap_arms(np.array(GOLD["episode_stats_in"]["action"]["max"])), np.array(GOLD["episode_stats_out"]["action"]["max"]))


# ------------------------------------------------------------------------------------------------ space mirroring: the views
def test_with_mirror_samples(root):
    ds = _windows(root)
    both = lrd.with_mirror(ds)
    n = len(ds)
    assert n == 18 and len(both) == 2 * n and len(lrd.MirroredView(ds)) == n
    for i in (0, 6, 7, 12, 17):
        _same(both[i], ds[i])  # i < len: the original sample
        raw, mir = ds[i], both[n + i]
        want = _hand_mirror(raw)
        want["episode_index"] = raw["episode_index"] + 3  # past the three original episodes, as a merge renumbers them
        _same(mir, want)
        ep, fr = (0, i) if i < 7 else (1, i - 7) if i < 17 else (2, 0)
        # pixel exact, against the generator: hand_left shows the flipped hand_right image
        assert np.array_equal(_pixels(mir["observation.images.top_head"]), _image(ep, fr, 0)[:, ::-1])
        assert np.array_equal(_pixels(mir["observation.images.hand_left"]), _image(ep, fr, 2)[:, ::-1])
        assert np.array_equal(_pixels(mir["observation.images.hand_right"]), _image(ep, fr, 1)[:, ::-1])
        assert not np.array_equal(_image(ep, fr, 0), _image(ep, fr, 0)[:, ::-1])
        assert np.array_equal(mir["observation.state"].numpy(), np.concatenate([_state(ep, fr)[7:], _state(ep, fr)[:7]]))
        assert torch.equal(mir["action_is_pad"], raw["action_is_pad"]) and mir["task"] == raw["task"]
        for key in ("timestamp", "frame_index", "index", "task_index", "progress_gt"):
            assert torch.equal(mir[key], raw[key])
    assert both[-1]["episode_index"] == 5 and int(lrd.MirroredView(ds)[3]["episode_index"]) == 0
    with pytest.raises(IndexError):
        both[2 * n]
    plan = lrd.view_plan(both)
    assert plan.frame_idx.tolist() == list(range(n)) * 2 and plan.frame_mirror.tolist() == [0] * n + [1] * n
    assert plan.frame_idx.dtype == plan.frame_stride.dtype == np.int32 and plan.frame_mirror.dtype == np.uint8 and not plan.is_identity
    assert lrd.view_plan(ds).is_identity
    # a vector that is not left + right long is an error, as in the reference
    with pytest.raises(ValueError, match="Array dimension mismatch: expected 13 dims"):
        lrd.MirroredView(ds, 6, 7)[0]
    # cameras outside the three roles: an error unless listed as flip-only (the reference drops them silently)
    cams = [f"observation.images.{c}" for c in CAMS]
    with pytest.raises(ValueError, match="wrist_cam"):
        lrd.camera_mirror_map([*cams, "observation.images.wrist_cam"])
    assert lrd.camera_mirror_map([*cams, "observation.images.wrist_cam"], flip_only=("wrist_cam",))["observation.images.wrist_cam"] == "observation.images.wrist_cam"
    with pytest.raises(ValueError, match="no counterpart"):
        lrd.camera_mirror_map(cams[:2])


def test_mirror_of_the_advantage_dataset(root):
    ds = lrd.AdvantageLerobotDataset(root, episodes=[0, 1], delta_timestamps={"action": [0.0, 1 / FPS]})
    mirrored = lrd.with_mirror(ds)
    assert len(mirrored) == 34
    for i in (0, 5, 16):
        random.seed(i)
        raw = ds[i]
        random.seed(i)  # the same comparison frame is drawn
        mir = mirrored[17 + i]
        want = _hand_mirror(raw, prefixes=("", "his_-100_"))
        want["episode_index"], want["his_-100_episode_index"] = raw["episode_index"] + 2, raw["his_-100_episode_index"] + 2
        _same(mir, want)
        assert mir["progress"] == raw["progress"] and mir["episode_length"] == raw["episode_length"]
        fr = int(raw["his_-100_frame_index"])
        ep = int(raw["episode_index"])
        assert np.array_equal(_pixels(mir["his_-100_observation.images.hand_left"]), _image(ep, fr, 2)[:, ::-1])
        assert np.array_equal(mir["his_-100_observation.state"].numpy(), np.concatenate([_state(ep, fr)[7:], _state(ep, fr)[:7]]))


# ------------------------------------------------------------------------------------------------ time scaling
KEPT = {2: [[0, 2, 4, 6], [0, 2, 4, 6, 8], [0]], 3: [[0, 3, 6], [0, 3, 6, 9], [0]]}  # range(0, L, N) for L = 7, 10, 1


@pytest.mark.parametrize("factor", [2, 3])
def test_time_scaling_samples(root, factor):
    ds = _windows(root, time_scaling=lrd.TimeScaling(factor))
    kept = KEPT[factor]
    assert [len(k) for k in kept] == [-(-n // factor) for n in LENGTHS] == ([4, 5, 1] if factor == 2 else [3, 4, 1])  # L < N keeps row 0
    assert len(ds) == sum(len(k) for k in kept) and ds.num_episodes == ds.num_view_episodes == 3
    plain = _windows(root)
    k = 0
    for ep, rows in enumerate(kept):
        for j, fr in enumerate(rows):
            it, raw = ds[k], plain[STARTS[ep] + fr]
            assert int(it["frame_index"]) == j and it["frame_index"].dtype == raw["frame_index"].dtype
            assert it["timestamp"].dtype == torch.float32 and float(it["timestamp"]) == float(np.float32(j / FPS))
            assert int(it["episode_index"]) == ep and int(it["index"]) == STARTS[ep] + fr  # every other column: original row j * N
            assert np.array_equal(it["observation.state"].numpy(), _state(ep, fr)) and it["task"] == raw["task"]
            for c, cam in enumerate(CAMS):  # the recorded frame of row j * N
                assert np.array_equal(_pixels(it[f"observation.images.{cam}"]), _image(ep, fr, c))
            # chunk row h is kept frame min(j + h, L' - 1); the flags are set past it
            want = [rows[min(j + h, len(rows) - 1)] for h in range(HORIZON)]
            assert np.array_equal(it["action"].numpy(), np.stack([_action(ep, f) for f in want]))
            assert it["action_is_pad"].tolist() == [j + h > len(rows) - 1 for h in range(HORIZON)]
            k += 1
    # literal: episode 0 (L = 7) at kept frame 2, horizon 5
    it = ds[2]
    if factor == 2:
        assert np.allclose(it["action"][:, 0].numpy() + 1.0, [0.04, 0.06, 0.06, 0.06, 0.06]) and it["action_is_pad"].tolist() == [False, False, True, True, True]
    else:
        assert np.allclose(it["action"][:, 0].numpy() + 1.0, [0.06] * 5) and it["action_is_pad"].tolist() == [False, True, True, True, True]
    plan = lrd.view_plan(ds)
    assert plan.frame_idx.tolist() == [STARTS[ep] + fr for ep, rows in enumerate(kept) for fr in rows]
    assert plan.frame_stride.tolist() == [factor] * len(ds) and not plan.frame_mirror.any()
    with pytest.raises(IndexError):
        ds[len(ds)]


def test_time_scaling_split_union_and_errors(root):
    # max(1, int(3 * 0.3)) = max(1, int(3 * 0.5)) = 1: the first episode BY INDEX is scaled and replaces its original
    for ratio in (0.3, 0.5):
        assert lrd.scaled_episode_positions([0, 1, 2], lrd.TimeScaling(2, ratio)) == [0]
        assert lrd.scaled_episode_positions([2, 0, 1], lrd.TimeScaling(2, ratio)) == [1]
    assert lrd.scaled_episode_positions(list(range(10)), lrd.TimeScaling(2, 0.3)) == [0, 1, 2]
    assert lrd.scaled_episode_positions(list(range(10)), lrd.TimeScaling(2, 0.99)) == list(range(9))
    assert lrd.scaled_episode_positions([4, 7], lrd.TimeScaling(3)) == [0, 1]
    ds = _windows(root, time_scaling=lrd.TimeScaling(2, 0.3))
    assert len(ds) == 4 + 10 + 1 and [int(ds[i]["index"]) for i in range(6)] == [0, 2, 4, 6, 7, 8]
    assert lrd.view_plan(ds).frame_stride.tolist() == [2] * 4 + [1] * 11
    _same(ds[4], {**_windows(root)[7]})  # an unscaled episode's samples are the original ones
    ds = _windows(root, episodes=[2, 1, 0], time_scaling=lrd.TimeScaling(2, 0.5))  # dataset order 2, 1, 0: episode 0 sits last
    assert len(ds) == 1 + 10 + 4 and [int(ds[i]["index"]) for i in (11, 12, 13, 14)] == [0, 2, 4, 6]
    # every episode scaled, the originals appended and renumbered past them
    ds = _windows(root, time_scaling=lrd.TimeScaling(2, union_original=True))
    assert len(ds) == 10 + 18 and ds.num_view_episodes == 6
    assert [int(ds[i]["episode_index"]) for i in (0, 4, 9, 10, 17, 27)] == [0, 1, 2, 3, 4, 5] and int(ds[10]["frame_index"]) == 0
    assert lrd.view_plan(ds).frame_idx.tolist() == [0, 2, 4, 6, 7, 9, 11, 13, 15, 17, *range(18)]
    assert lrd.with_mirror(ds)[28]["episode_index"] == 6
    # factor 1 keeps every row
    ds1 = _windows(root, time_scaling=lrd.TimeScaling(1))
    assert len(ds1) == 18
    _same(ds1[9], _windows(root)[9])
    for bad in (dict(factor=0), dict(factor=2.0), dict(factor=2, split_ratio=0.0), dict(factor=2, split_ratio=1.0),
                dict(factor=2, split_ratio=0.3, union_original=True)):  # fmt: skip
        with pytest.raises(ValueError):
            lrd.TimeScaling(**bad)


def test_time_scaled_advantage_dataset(root):
    ds = lrd.AdvantageLerobotDataset(root, episodes=[0, 1], delta_timestamps={"action": [0.0, 1 / FPS]}, time_scaling=lrd.TimeScaling(3))
    assert len(ds) == 3 + 4
    random.seed(1)
    for i in range(len(ds)):
        it = ds[i]
        ep = int(it["episode_index"])
        assert it["episode_length"] == (3, 4)[ep] and int(it["his_-100_episode_index"]) == ep
        j, other = int(it["frame_index"]), int(it["his_-100_frame_index"])
        assert 0 <= other < (3, 4)[ep] and other != j
        assert np.array_equal(it["his_-100_observation.state"].numpy(), _state(ep, 3 * other))  # a kept, recorded frame
        assert abs(it["progress"] - (float(it["stage_progress_gt"]) - float(it["his_-100_stage_progress_gt"]))) < 1e-7


# ------------------------------------------------------------------------------------------------ configs, transforms, statistics
def _train_config(root, assets, factory=tc.LerobotAgilexDataConfig, **kw):
    from tiny import tiny_cfgs

    pcfg, _ = tiny_cfgs(action_horizon=HORIZON, max_token_len=96)
    return tc.TrainConfig(name="tiny_augment", exp_name="t", model=pcfg, batch_size=4, num_workers=0, assets_base_dir=str(assets),
                          data=factory(repo_id=str(root), default_prompt="Flatten and fold the cloth.", tokenizer_model=_tok(), **kw))  # fmt: skip


class _One:
    def __init__(self, item):
        self.item = item

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return dict(self.item)


def test_config_fields_reach_the_datasets(root, tmp_path):
    for factory in (tc.LerobotAgilexDataConfig, tc.LerobotARXDataConfig):
        names = {f.name: f.default for f in dataclasses.fields(factory)}
        assert (names["space_mirror"], names["time_scaling"], names["left_dim"], names["right_dim"]) == (False, None, 7, 7)
    cfg = _train_config(root, tmp_path / "assets")
    dc = cfg.data.create(cfg.assets_dirs, cfg.model)
    assert dc.space_mirror is False and dc.time_scaling is None
    plain = lrd.create_torch_dataset(dc, HORIZON, cfg.model)
    assert type(plain) is lrd.LeRobotDataset and plain._view is None and len(plain) == 18  # no wrapper, no view: the same object as before
    direct = _windows(root)
    for i in range(18):
        _same(plain[i], direct[i])
    aug = _train_config(root, tmp_path / "assets", factory=tc.LerobotARXDataConfig, space_mirror=True, time_scaling=lrd.TimeScaling(2, 0.3))
    adc = aug.data.create(aug.assets_dirs, aug.model)
    assert adc.space_mirror and adc.time_scaling == tc.TimeScaling(2, 0.3) and tc.TimeScaling is lrd.TimeScaling
    ds = lrd.create_torch_dataset(adc, HORIZON, aug.model)
    assert len(ds) == 30 and lrd.view_plan(ds).frame_mirror.tolist() == [0] * 15 + [1] * 15
    _same(lrd.view_plan(ds).__dict__, lrd.plan_view(LENGTHS, [0, 1, 2], lrd.TimeScaling(2, 0.3), True).__dict__)  # loader and norm stats: one plan
    # time scaling first, mirroring over the result: sample 15 + k is the mirror of time-scaled sample k
    scaled = _windows(root, time_scaling=lrd.TimeScaling(2, 0.3))
    want = _hand_mirror(scaled[2])
    want["episode_index"] = scaled[2]["episode_index"] + 3
    _same(ds[17], want)
    assert int(ds[17]["frame_index"]) == 2 and int(ds[17]["index"]) == 4
    adv = lrd.create_advantage_torch_dataset(adc, HORIZON, aug.model, dataclasses.replace(aug, advantage_estimator=True))
    assert len(adv) == 30 and isinstance(lrd._base_dataset(adv), lrd.AdvantageLerobotDataset)
    # the override form of cli(): dotted names, as tyro spells nested fields
    got = tc.cli(["pi05_flatten_fold_normal", "--data.space_mirror", "--data.time_scaling.factor", "3", "--data.time_scaling.split_ratio", "0.5",
                  "--batch_size", "8"])  # fmt: skip
    assert got.data.space_mirror and got.data.time_scaling == tc.TimeScaling(3, 0.5) and got.batch_size == 8 and got.data.left_dim == 7
    assert tc.cli(["pi05_hang_cloth_normal", "--data.left-dim", "6", "--data.right-dim", "8"]).data.right_dim == 8
    assert tc.cli(["pi05_flatten_fold_normal"]) is not None and tc.cli(["pi05_flatten_fold_normal"]).data == tc.get_config("pi05_flatten_fold_normal").data


@pytest.mark.parametrize("delta", [True, False])
def test_mirrored_sample_through_the_transform_stack(root, tmp_path, delta):
    """The swap happens on the raw sample, so everything downstream sees a mirrored parquet row: pi0.5's discretised state in the
    prompt is the swapped state, and DeltaActions subtracts the swapped state from the swapped actions."""
    cfg = _train_config(root, tmp_path / "assets", space_mirror=True, time_scaling=lrd.TimeScaling(2, 0.3), use_delta_joint_actions=delta)
    assert cfg.model.discrete_state_input
    rng = np.random.default_rng(0)
    stats = {k: normalize.NormStats(mean=rng.normal(size=32), std=rng.uniform(0.5, 2, size=32), q01=-rng.uniform(1, 2, size=32), q99=rng.uniform(1, 2, size=32))
             for k in ("state", "actions")}  # fmt: skip
    dc = dataclasses.replace(cfg.data.create(cfg.assets_dirs, cfg.model), norm_stats=stats)
    full = lrd.transform_dataset(lrd.create_torch_dataset(dc, HORIZON, cfg.model), dc)
    scaled = _windows(root, time_scaling=lrd.TimeScaling(2, 0.3))
    for k in (0, 3, 9, 14):
        by_hand = lrd.transform_dataset(_One(_hand_mirror(scaled[k])), dc)[0]
        got = full[15 + k]
        _same(got, by_hand)
        assert not np.array_equal(np.asarray(got["tokenized_prompt"]), np.asarray(full[k]["tokenized_prompt"]))  # the state tokens moved
        assert not np.array_equal(np.asarray(got["actions"]), np.asarray(full[k]["actions"]))
    if delta:  # written out: actions[..., c] - state[c] on the swapped row, for the columns of make_bool_mask(6, -1, 6, -1)
        raw = _hand_mirror(scaled[3])
        robot = TransformedDataset(lrd.create_torch_dataset(dc, HORIZON, cfg.model), [*dc.repack_transforms.inputs, *dc.data_transforms.inputs])[18]
        mask = np.array([True] * 6 + [False] + [True] * 6 + [False])
        want = raw["action"].numpy() - np.where(mask, raw["observation.state"].numpy(), np.float32(0))
        assert np.array_equal(np.asarray(robot["actions"])[:, :14], want)


def test_chunk_rows_and_host_stats_over_a_view(root, tmp_path):
    state, action, ep_end = lrd.read_state_action_columns(root, "observation.state", "action")
    assert np.array_equal(state[8], _state(1, 1)) and ep_end.tolist() == [7] * 7 + [17] * 10 + [18]
    state, action = state.copy(), action.copy()
    action[[3, 9, 16], [2, 9, 12]] = [3.5, -4.0, 3.2]  # glitches on both arms, in the tables only (chunk_rows against itself below)
    kw = dict(horizon=HORIZON, action_dim=32, clip_state=True, clip_action=True, mask_state=False, delta_mask=0b01111110111111)
    # None views: today's function, restated here line by line
    idx = np.array([16, 0, 3, 3, 8, 17])
    for frame_idx in (None, idx):
        got_s, got_a = ns.chunk_rows(state, action, ep_end, frame_idx=frame_idx, **kw)
        i = np.arange(18) if frame_idx is None else frame_idx
        rows = np.minimum(i[:, None] + np.arange(HORIZON)[None, :], ep_end[i].astype(np.int64)[:, None] - 1)
        s = np.pad(state[i], ((0, 0), (0, 18)))
        s = np.where(np.abs(s) > ns.PI_F32, np.float32(0), s)
        a = np.pad(action[rows], ((0, 0), (0, 0), (0, 18)))
        a = np.where(np.abs(a) > ns.PI_F32, np.float32(0), a)
        m = np.array([(kw["delta_mask"] >> c) & 1 for c in range(32)], bool)
        a = a - np.where(m, s, np.float32(0))[:, None, :]
        assert got_s.tobytes() == s.astype(np.float32).tobytes() and got_a.tobytes() == a.astype(np.float32).tobytes()
        ones, zeros = np.ones(len(i), np.int32), np.zeros(len(i), np.uint8)
        for view in (dict(frame_stride=ones), dict(frame_mirror=zeros), dict(frame_stride=ones, frame_mirror=zeros)):
            again = ns.chunk_rows(state, action, ep_end, frame_idx=frame_idx, **kw, **view)
            assert again[0].tobytes() == got_s.tobytes() and again[1].tobytes() == got_a.tobytes()
    # literal: frame 4 of episode 0 at stride 2 -> rows 4, 6, 6, 6, 6; frame 3 at stride 3 -> 3, 6, 6, ... (6 is kept from 3);
    # frame 2 at stride 3 -> 2, 5, 5, ... (the last row kept FROM 2, not the episode's last row)
    _, a = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=14, clip_state=False, clip_action=False, mask_state=False,
                         delta_mask=0, frame_idx=np.array([4, 3, 2]), frame_stride=np.array([2, 3, 3]))  # fmt: skip
    assert [[int(np.flatnonzero((action == r).all(1))[0]) for r in chunk] for chunk in a] == [[4, 6, 6, 6, 6], [3, 6, 6, 6, 6], [2, 5, 5, 5, 5]]
    # the mirror permutes BEFORE clip and delta: equal to the plain function on a table whose arms were swapped on disk
    perm = normalize.arm_swap_perm(14)
    flags = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    got_s, got_a = ns.chunk_rows(state, action, ep_end, frame_idx=idx, frame_mirror=flags, **kw)
    swapped = ns.chunk_rows(state[:, perm], action[:, perm], ep_end, frame_idx=idx, **kw)
    plain = ns.chunk_rows(state, action, ep_end, frame_idx=idx, **kw)
    for got, sw, pl in ((got_s, swapped[0], plain[0]), (got_a, swapped[1], plain[1])):
        assert np.array_equal(got[flags == 1], sw[flags == 1]) and np.array_equal(got[flags == 0], pl[flags == 0])
        assert not np.array_equal(got, pl)
    with pytest.raises(ValueError, match="Insufficient array dimensions"):
        ns.chunk_rows(state, action, ep_end, horizon=2, action_dim=14, clip_state=False, clip_action=False, mask_state=False, delta_mask=0,
                      frame_mirror=np.ones(18, np.uint8), left_dim=8, right_dim=7)  # fmt: skip
    # host_stats over the plan == the one-shot estimator over the rows gathered by iterating the augmented, transformed dataset
    for extra in (dict(space_mirror=True), dict(time_scaling=lrd.TimeScaling(3)), dict(space_mirror=True, time_scaling=lrd.TimeScaling(2, 0.3))):
        cfg = _train_config(root, tmp_path / "assets", use_delta_joint_actions=True, **extra)
        dc = cfg.data.create(cfg.assets_dirs, cfg.model)
        spec = ns.lower_transforms(dc)
        ds = lrd.create_torch_dataset(dc, HORIZON, cfg.model)
        robot = TransformedDataset(ds, [*dc.repack_transforms.inputs, *dc.data_transforms.inputs])
        samples = [robot[i] for i in range(len(robot))]
        plan = lrd.view_plan(ds)
        s_read, a_read, e_read = lrd.read_state_action_columns(root, spec.state_col, spec.action_col)
        got = ns.host_stats(s_read, a_read, e_read, spec, HORIZON, plan.frame_idx, frame_stride=plan.frame_stride, frame_mirror=plan.frame_mirror)
        slabbed = ns.host_stats(s_read, a_read, e_read, spec, HORIZON, plan.frame_idx, frame_stride=plan.frame_stride,
                                frame_mirror=plan.frame_mirror, slab_rows=20)  # fmt: skip
        whole = ns.compute_norm_stats(cfg, device="cpu")
        for key in ns.KEYS:
            want = ns.one_shot(np.stack([np.asarray(x[key]) for x in samples]))
            for f in ("mean", "std", "q01", "q99"):
                assert np.array_equal(getattr(got[key], f), getattr(want, f)), (extra, key, f)
                assert np.array_equal(getattr(whole[key], f), getattr(want, f)), (extra, key, f)
            assert np.array_equal(slabbed[key].q01, want.q01) and np.array_equal(slabbed[key].q99, want.q99)
            assert np.allclose(slabbed[key].mean, want.mean, rtol=0, atol=1e-14) and np.allclose(slabbed[key].std, want.std, rtol=0, atol=1e-12)
    # mirroring the statistics of the original is NOT the statistics of the union: that is why they are computed over the view
    base = ns.compute_norm_stats(_train_config(root, tmp_path / "assets", use_delta_joint_actions=True), device="cpu")
    assert not np.array_equal(normalize.mirror_norm_stats(base)["actions"].mean, whole["actions"].mean)


def test_cli_writes_the_statistics_of_the_augmented_dataset(root, tmp_path, monkeypatch):
    from kai0_amd import compute_norm_stats as cli

    cfg = dataclasses.replace(_train_config(root, tmp_path / "assets", space_mirror=True, time_scaling=lrd.TimeScaling(2, 0.3)), name="tiny_augment_cli")
    monkeypatch.setitem(tc._CONFIGS_DICT, cfg.name, cfg)
    path = cli.main([cfg.name, "--host"])
    loaded = cfg.data.create(cfg.assets_dirs, cfg.model).norm_stats
    assert path.exists() and loaded is not None
    want = ns.compute_norm_stats(cfg, device="cpu")
    plain = ns.compute_norm_stats(dataclasses.replace(cfg, data=dataclasses.replace(cfg.data, space_mirror=False, time_scaling=None)), device="cpu")
    for key in ns.KEYS:
        assert np.array_equal(loaded[key].q99, want[key].q99) and np.array_equal(loaded[key].mean, want[key].mean)
    assert np.array_equal(loaded["actions"].q99[:7], loaded["actions"].q99[7:14]) and not np.array_equal(plain["actions"].q99[:7], plain["actions"].q99[7:14])
    # --max-frames samples the AUGMENTED sample list
    sub = ns.compute_norm_stats(cfg, max_frames=12, seed=5, device="cpu")
    pick = np.sort(np.random.default_rng(5).choice(30, size=12, replace=False))
    plan = lrd.plan_view(LENGTHS, None, lrd.TimeScaling(2, 0.3), True)
    s_read, a_read, e_read = lrd.read_state_action_columns(root, "observation.state", "action")
    rows = ns.chunk_rows(s_read, a_read, e_read, horizon=HORIZON, action_dim=32, clip_state=True, clip_action=True, mask_state=False,
                         delta_mask=0b01111110111111, frame_idx=plan.frame_idx[pick], frame_stride=plan.frame_stride[pick],
                         frame_mirror=plan.frame_mirror[pick])[1]  # fmt: skip
    assert np.array_equal(sub["actions"].q99, ns.one_shot(rows).q99)
