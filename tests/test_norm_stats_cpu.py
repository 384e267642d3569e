"""Normalisation statistics on the host (kai0_amd/norm_stats.py): `chunk_rows` against the real transform stack bit for bit,
`lower_transforms`, the CLI's file round trip, constant / padded columns, and the documented gap between the one-shot estimator and
the reference script's streamed form."""

import dataclasses
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import norm_stats_refs as refs  # noqa: E402
from kai0_amd import lerobot_dataset as lrd  # noqa: E402
from kai0_amd import norm_stats as ns  # noqa: E402
from kai0_amd import normalize  # noqa: E402
from kai0_amd import training_config as tc  # noqa: E402
from kai0_amd import transforms  # noqa: E402
from kai0_amd.data_loader import TransformedDataset  # noqa: E402

LENGTHS = [1, 2, 5, 9]
HORIZON = 4
CAMS = ("top_head", "hand_left", "hand_right")
CONFIGS = {"agilex_delta": (tc.LerobotAgilexDataConfig, dict(use_delta_joint_actions=True)),
           "agilex_abs": (tc.LerobotAgilexDataConfig, dict(use_delta_joint_actions=False)),
           "arx": (tc.LerobotARXDataConfig, dict(use_delta_joint_actions=True)),
           "mask_state": (tc.LerobotAgilexDataConfig, dict(use_delta_joint_actions=True, mask_state=True))}  # fmt: skip


def _tok():
    return np.load(os.path.join(HERE, "golden", "host_pipeline.npz"))["tok.model"].tobytes()


def _tables():
    state, action, ep_end = refs.random_walk_table(LENGTHS, seed=3, scale=0.4)
    refs.boundary_values(state, action)
    return state, action, ep_end


def _train_config(root, assets, factory=tc.LerobotAgilexDataConfig, name="tiny_stats", **kw):
    from tiny import tiny_cfgs

    pcfg, _ = tiny_cfgs(action_horizon=HORIZON, max_token_len=64)
    return tc.TrainConfig(name=name, exp_name="t", model=pcfg, batch_size=4, num_workers=0, assets_base_dir=str(assets),
                          data=factory(repo_id=str(root), default_prompt="Flatten and fold the cloth.", tokenizer_model=_tok(), **kw))  # fmt: skip


@dataclasses.dataclass(frozen=True)
class AddCameras:
    """The test dataset has no camera feature; AgilexInputs insists on its three cameras."""

    def __call__(self, data):
        return {**data, **{f"observation.images.{c}": np.zeros((3, 2, 2), np.float32) for c in CAMS}}


@dataclasses.dataclass(frozen=True)
class ScaleActions:
    """A robot transform `lower_transforms` does not know."""

    def __call__(self, data):
        return {"state": np.asarray(data["state"], np.float32) * 2, "actions": np.asarray(data["actions"], np.float32) * 3}


@dataclasses.dataclass(frozen=True)
class UnknownDataConfig(tc.DataConfigFactory):
    def create(self, assets_dirs, model_config):
        return dataclasses.replace(self.create_base_config(assets_dirs, model_config), action_sequence_keys=("action",),
                                   repack_transforms=transforms.Group(inputs=[transforms.RepackTransform(
                                       {"state": "observation.state", "actions": "action"})]),
                                   data_transforms=transforms.Group(inputs=[ScaleActions()]))  # fmt: skip


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    state, action, ep_end = _tables()
    root = refs.write_dataset(tmp_path_factory.mktemp("ds") / "FlattenFold", LENGTHS, state, action)
    return root, state, action, ep_end


@pytest.mark.parametrize("which", list(CONFIGS))
def test_chunk_rows_equals_the_transform_stack_bit_for_bit(dataset, tmp_path, which):
    root, state, action, ep_end = dataset
    factory, kw = CONFIGS[which]
    cfg = _train_config(root, tmp_path / "assets", factory, **kw)
    dc = cfg.data.create(cfg.assets_dirs, cfg.model)
    spec = ns.lower_transforms(dc)
    assert spec is not None and (spec.state_col, spec.action_col, spec.action_dim) == ("observation.state", "action", 32)
    assert spec.clip_action and spec.clip_state == (which != "arx") and spec.mask_state == (which == "mask_state")
    assert spec.delta_mask == (0 if which == "agilex_abs" else 0b01111110111111)
    # the light reader returns the tables as written, with the episode ends
    s_read, a_read, e_read = lrd.read_state_action_columns(root, spec.state_col, spec.action_col)
    assert s_read.tobytes() == state.tobytes() and a_read.tobytes() == action.tobytes() and np.array_equal(e_read, ep_end)
    assert s_read.dtype == a_read.dtype == np.float32 and e_read.dtype == np.int32
    ds = TransformedDataset(lrd.create_torch_dataset(dc, HORIZON, cfg.model),
                            [AddCameras(), *dc.repack_transforms.inputs, *dc.data_transforms.inputs])  # fmt: skip
    want_s = np.stack([np.asarray(ds[i]["state"]) for i in range(len(ds))])
    want_a = np.stack([np.asarray(ds[i]["actions"]) for i in range(len(ds))])
    got_s, got_a = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=spec.action_dim, clip_state=spec.clip_state,
                                 clip_action=spec.clip_action, mask_state=spec.mask_state, delta_mask=spec.delta_mask)  # fmt: skip
    assert want_s.dtype == want_a.dtype == np.float32 and got_s.shape == (17, 32) and got_a.shape == (17, HORIZON, 32)
    # bit for bit up to the sign of zero (where(|x| > pi, 0, x) and x - x produce +0.0 either way; -0.0 passes through both)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_a, want_a)
    assert np.array_equal(np.signbit(got_s), np.signbit(want_s)) and np.array_equal(np.signbit(got_a), np.signbit(want_a))
    # the boundary is really in play: f32(pi) survives the filter, the next f32 and the 4.0 glitch do not
    if which == "agilex_abs":
        flat = np.abs(got_a).ravel()
        assert (flat == refs.PI32).any() and not (flat > refs.PI32).any() and (np.abs(action) > refs.PI32).sum() >= 4
    if which == "arx":
        assert (np.abs(got_s) > refs.PI32).any()  # ARXInputs does not filter the state
    # a subset in any order, with duplicates
    idx = np.array([16, 0, 3, 3, 8, 1])
    sub_s, sub_a = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=32, clip_state=spec.clip_state, clip_action=True,
                                 mask_state=spec.mask_state, delta_mask=spec.delta_mask, frame_idx=idx)  # fmt: skip
    assert np.array_equal(sub_s, want_s[idx]) and np.array_equal(sub_a, want_a[idx])


def test_lower_transforms_refuses_what_it_does_not_know(dataset, tmp_path):
    root, state, action, ep_end = dataset
    cfg = _train_config(root, tmp_path / "assets", insert_advantage_into_prompt=True)
    assert ns.lower_transforms(cfg.data.create(cfg.assets_dirs, cfg.model)) is not None  # InsertAdvantageIntoPrompt: neither key
    from tiny import tiny_cfgs

    pcfg, _ = tiny_cfgs(action_horizon=HORIZON, max_token_len=64)
    unknown = tc.TrainConfig(name="tiny_unknown", exp_name="t", model=pcfg, batch_size=4, num_workers=0,
                             assets_base_dir=str(tmp_path / "assets"), data=UnknownDataConfig(repo_id=str(root)))  # fmt: skip
    dc = unknown.data.create(unknown.assets_dirs, unknown.model)
    assert ns.lower_transforms(dc) is None
    wide = dataclasses.replace(pcfg, action_dim=33)
    assert ns.lower_transforms(tc.LerobotAgilexDataConfig(repo_id=str(root), tokenizer_model=_tok()).create(tmp_path, wide)) is None
    # ... and still gets its statistics, through the transformed dataset
    stats = ns.compute_norm_stats(unknown, device="cpu")
    rs = {k: normalize.RunningStats() for k in ("state", "actions")}
    rows_s, rows_a = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=14, clip_state=False, clip_action=False,
                                   mask_state=False, delta_mask=0)  # fmt: skip
    for i in range(0, 17, 4):
        rs["state"].update(rows_s[i : i + 4] * np.float32(2))
        rs["actions"].update(rows_a[i : i + 4] * np.float32(3))
    for k in rs:
        want = rs[k].get_statistics()
        for f in ("mean", "std", "q01", "q99"):
            assert np.array_equal(getattr(stats[k], f), getattr(want, f)), (k, f)


def test_cli_writes_the_file_the_factory_loads(dataset, tmp_path, monkeypatch, capsys):
    from kai0_amd import compute_norm_stats as cli

    root, state, action, ep_end = dataset
    cfg = _train_config(root, tmp_path / "assets", name="tiny_stats_cli", use_delta_joint_actions=True)
    monkeypatch.setitem(tc._CONFIGS_DICT, cfg.name, cfg)
    assert cfg.data.create(cfg.assets_dirs, cfg.model).norm_stats is None
    with pytest.raises(ValueError, match="Normalization stats not found. Make sure to run `python -m kai0_amd.compute_norm_stats"):
        lrd.transform_dataset(None, cfg.data.create(cfg.assets_dirs, cfg.model))
    path = cli.main([cfg.name, "--host"])
    assert path == cfg.assets_dirs / str(root) / "norm_stats.json" and path.exists() and str(path) in capsys.readouterr().out
    loaded = tc.get_config(cfg.name).data.create(cfg.assets_dirs, cfg.model).norm_stats
    s, a = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=32, clip_state=True, clip_action=True, mask_state=False,
                         delta_mask=0b01111110111111)  # fmt: skip
    for key, rows in (("state", s), ("actions", a)):
        rs = normalize.RunningStats()
        rs.update(rows.astype(np.float64))
        want = rs.get_statistics()
        for f in ("mean", "std", "q01", "q99"):
            assert np.array_equal(getattr(loaded[key], f), getattr(want, f)), (key, f)
            assert getattr(loaded[key], f).shape == (32,)
    # --max-frames: a seeded sample without replacement, the same one every time
    sub = ns.compute_norm_stats(cfg, max_frames=9, seed=5, device="cpu")
    idx = np.sort(np.random.default_rng(5).choice(17, size=9, replace=False))
    want = ns.one_shot(ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=32, clip_state=True, clip_action=True,
                                     mask_state=False, delta_mask=0b01111110111111, frame_idx=idx)[1])  # fmt: skip
    assert np.array_equal(sub["actions"].q99, want.q99) and np.array_equal(sub["actions"].mean, want.mean)


def test_constant_and_padded_columns_get_the_estimators_answer():
    """Columns with lo == hi never reach the histogram pass: the finishing code places their count where np.histogram would, so
    the full-width result equals RunningStats on the full-width rows — through the slabbed two-pass form too."""
    state, action, ep_end = refs.random_walk_table([5, 40, 23], seed=1)
    action[:, 13] = 0.07  # a stuck gripper
    action[:, 2] = -0.0
    spec = ns.ChunkSpec("s", "a", 32, True, True, True, 0b01111110111111)  # masked state: all 32 state columns constant
    whole = ns.host_stats(state, action, ep_end, spec, 7)
    slabbed = ns.host_stats(state, action, ep_end, spec, 7, slab_rows=50)
    s, a = ns.chunk_rows(state, action, ep_end, horizon=7, action_dim=32, clip_state=True, clip_action=True, mask_state=True,
                         delta_mask=spec.delta_mask)  # fmt: skip
    for key, rows in (("state", s), ("actions", a.reshape(-1, 32))):
        ref = refs.Reference(rows)
        for got in (whole[key], slabbed[key]):
            ref.check_stats(got, key)
        assert np.array_equal(whole[key].mean, ref.stats.mean) and np.array_equal(whole[key].std, ref.stats.std)
        const = ref.lo == ref.hi
        assert const.sum() >= (32 if key == "state" else 20)
        assert np.array_equal(slabbed[key].q01[const], ref.stats.q01[const])
    with pytest.raises(ValueError, match=r"key 'actions', column 4 "):
        bad = action.copy()
        bad[17, 4] = np.nan
        ns.host_stats(state, bad, ep_end, spec, 7)
    with pytest.raises(ValueError, match=r"key 'actions', column 4 "):
        ns.host_stats(state, bad, ep_end, spec, 7, slab_rows=50)


def test_entry_points_validate_on_the_host():
    """The two entry points check their arguments before anything is launched, so the checks run here; so does the workspace query
    (one {min, max, sum, sumsq} per block and column; blocks = ceil(M / 32) up to 1024)."""
    from kai0_amd import _lib

    lib = _lib.load()
    q = lib.kai0_chunk_stats_workspace_bytes
    assert (q(0, 32), q(1, 1), q(33, 14), q(12_000, 14), q(10**6, 32), q(5, 33), q(5, 0)) == (1024, 32, 2 * 14 * 32, 375 * 14 * 32, 1024 * 1024, -1, -1)
    ok = dict(state=8, ld_state=14, ds=14, action=8, ld_action=14, da=14, ep_end=8, N=10, frame_idx=None, M=10, horizon=50, width=32,
              clip_state=1, clip_action=1, mask_state=0, delta_mask=0x3F)  # fmt: skip
    tail_m, tail_h = (8, 8, 1 << 20, None), (8, 5000, 1, 8, None)
    for change, msg in ((dict(width=33), "width=33"), (dict(horizon=0), "horizon=0"), (dict(da=33), "da=33"), (dict(ld_state=13), "row stride 13"),
                        (dict(width=14, delta_mask=1 << 14), "selects a column >= width=14"), (dict(M=11), "without frame_idx"),
                        (dict(state=None), "null buffer"), (dict(action=6), "not aligned")):  # fmt: skip
        for name, tail in (("kai0_chunk_stats_moments", tail_m), ("kai0_chunk_stats_hist", tail_h)):
            with pytest.raises(_lib.Kai0HipError, match=msg):
                _lib.call(name, *{**ok, **change}.values(), *tail)
    with pytest.raises(_lib.Kai0HipError, match="needs an 8-byte aligned workspace of 1024 bytes"):
        _lib.call("kai0_chunk_stats_moments", *ok.values(), 8, 8, 1023, None)
    with pytest.raises(_lib.Kai0HipError, match="bins=40961"):
        _lib.call("kai0_chunk_stats_hist", *ok.values(), 8, 40961, 1, 8, None)
    with pytest.raises(_lib.Kai0HipError, match="col_mask"):
        _lib.call("kai0_chunk_stats_hist", *{**ok, "width": 14, "delta_mask": 0}.values(), 8, 5000, 1 << 14, 8, None)
    _lib.call("kai0_chunk_stats_hist", *{**ok, "M": 0}.values(), None, 5000, 1, None, None)  # nothing to do, nothing launched
    _lib.call("kai0_chunk_stats_hist", *ok.values(), None, 5000, 0, None, None)  # no column selected


def test_guess_and_fix_up_is_np_histogram():
    """The bin rule of kai0_chunk_stats_hist restated in numpy f64 — floor((x - e0) * bins / (eB - e0)), then moved until
    e[k] <= x < e[k + 1], the last bin closed — gives np.histogram's counts as integers, on wide, one-ulp-wide and offset ranges."""
    rng = np.random.default_rng(0)
    one = np.float32(1.0)
    cols = [rng.normal(0, 1, 20000), rng.uniform(1e-6, 3, 20000), np.where(rng.random(20000) < 0.5, 0.0, 0.07),
            np.array([one, np.nextafter(one, np.float32(2))] * 50), 1000.0 + rng.uniform(0, 1e-3, 20000)]  # fmt: skip
    for x in cols:
        x = x.astype(np.float32).astype(np.float64)
        e = np.linspace(x.min() - 1e-10, x.max() + 1e-10, 5001)
        want, _ = np.histogram(x, bins=e)
        k = np.clip(np.floor((x - e[0]) * (5000 / (e[-1] - e[0]))), 0, 4999).astype(np.int64)
        moved = 0
        while True:
            down, up = (k > 0) & (x < e[k]), (k < 4999) & (x >= e[np.minimum(k + 1, 5000)])
            if not (down | up).any():
                break
            k = k - down + (up & ~down)
            moved += 1
        assert moved <= 2 and np.array_equal(np.bincount(k, minlength=5000), want)


def test_gap_to_the_streamed_reference_form():
    """The reference script feeds RunningStats 32 frames at a time: whenever a batch widens a column's range the counts so far are
    re-binned from their old left edges (np.histogram(edges[:-1], new_edges, weights=hist)), which moves mass by less than one NEW
    bin per re-binning but can pile several old bins into one.  The one-shot form never re-bins.  Largest q01 / q99 gap on the
    12-episode random-walk table below, in bin widths of the one-shot edges: printed here, quoted in DESIGN.md §13.
    The assertion bounds the STREAMED form's smear (the reference's own property, not this code's): measured 2.00 bin widths on
    this table (the one-shot form itself sits 1.38 widths from np.quantile).  Each form reports an edge, so one width of the gap is
    quantisation; the rest is counts that a re-binning moved by up to one bin.  Twice the measurement, 4 widths, is the margin.  (The
    one-shot path's own yardstick is elsewhere: the bit-for-bit comparisons with RunningStats.)  The streamed form is fed f32 batches and keeps f32 batch means: measured
    8.7e-8 of the table's 1.5 rad scale, i.e. one f32 ulp; the margin is 1e-6 (eight f32 ulps: a batch mean carries half an ulp of
    rounding per pairwise level over 32 x 50 rows)."""
    lengths = [157, 230, 91, 310, 45, 188, 260, 77, 142, 201, 66, 119]
    state, action, ep_end = refs.random_walk_table(lengths, seed=12)
    _, a = ns.chunk_rows(state, action, ep_end, horizon=50, action_dim=14, clip_state=True, clip_action=True, mask_state=False,
                         delta_mask=0b01111110111111)  # fmt: skip
    one = normalize.RunningStats()
    one.update(a.astype(np.float64))
    streamed = normalize.RunningStats()
    for i in range(0, len(a), 32):
        streamed.update(a[i : i + 32])
    o, s = one.get_statistics(), streamed.get_statistics()
    width = np.array([e[1] - e[0] for e in one.edges])
    varying = width > 1e-12
    gap = np.maximum(np.abs(o.q01 - s.q01), np.abs(o.q99 - s.q99))[varying] / width[varying]
    exact = np.quantile(a.reshape(-1, 14).astype(np.float64), [0.01, 0.99], axis=0)
    own = np.maximum(np.abs(o.q01 - exact[0]), np.abs(o.q99 - exact[1]))[varying] / width[varying]
    rel_mean = np.max(np.abs(o.mean - s.mean) / 1.5)
    print(f"one-shot vs streamed(32): q01/q99 gap {gap.max():.2f} bin widths, mean gap {rel_mean:.2e} of the 1.5 rad scale; "
          f"one-shot vs the exact quantile {own.max():.2f} bin widths")
    assert gap.max() <= 4.0 and rel_mean <= 1e-6
    assert own.max() <= 2.0  # an edge next to the exact quantile: one width of quantisation, one of interpolation convention
