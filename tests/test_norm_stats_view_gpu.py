"""Normalisation statistics over a dataset VIEW on the MI355X (kai0_chunk_stats_moments_view / kai0_chunk_stats_hist_view through
kai0_amd.norm_stats): time scaling as a per-frame stride, space mirroring as a per-frame arm swap.  The reference of
every case is `chunk_rows` with the same view arguments (held to the loader's samples by tests/test_data_augment_cpu.py): min, max
and every histogram count exactly, the sums within (n - 1) 2^-53 sum|x| of the exact `math.fsum` value (norm_stats_refs.Reference:
the bound of ANY summation order, computed from the rows).  Fixed: width 16, ds = da = 14, horizon 5."""

import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import norm_stats_refs as refs  # noqa: E402
from kai0_amd import _lib  # noqa: E402
from kai0_amd import lerobot_dataset as lrd  # noqa: E402
from kai0_amd import norm_stats as ns  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTH, D, HORIZON = 16, 14, 5
SYMMETRIC = 0b01111110111111  # make_bool_mask(6, -1, 6, -1): the same columns of either arm
LEFT_ONLY = 0b00000000101011  # not symmetric under the swap: a mirrored frame subtracts RIGHT-arm state from these columns
GUARD = 8  # NaN rows in front of and behind each table, and NaN columns 14, 15 beside it


def _tables(lengths, seed):
    state, action, ep_end = refs.random_walk_table(lengths, seed=seed, scale=0.3)
    refs.boundary_values(state, action)
    for t in (state, action):  # |x| > pi on both arms, on top of what boundary_values plants
        t[len(t) // 2, 2], t[len(t) // 2, 9], t[-1, 5], t[0, 12] = 3.5, -3.5, 4.0, -4.0
    return state, action, ep_end


@pytest.fixture(scope="module")
def tables():
    """The three-episode table of the loader tests, and ~3 000 frames in episodes of 1..40 frames: the frames of a launch then
    cross block slabs (pass 1: 8 frames per block trip, pass 2: 128) and episode ends everywhere."""
    rng = np.random.default_rng(11)
    lengths = []
    while sum(lengths) < 3000:
        lengths.append(int(rng.integers(1, 41)))
    return {"small": _tables([7, 10, 1], seed=1), "large": _tables(lengths, seed=2)}


def _view(n, seed, m=None):
    """frame_idx out of order and with duplicates, strides 1 / 2 / 3 and mirror flags mixed per frame."""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, size=n // 4 + 3), [n - 1, n - 1, 0]]) if m is None else rng.integers(0, n, size=m)
    return idx.astype(np.int64), rng.integers(1, 4, size=len(idx)).astype(np.int32), (rng.random(len(idx)) < 0.5).astype(np.uint8)


def _guarded(table, dev):
    """The table inside a NaN frame: GUARD rows before and after, two NaN columns to its right.  A read outside the table puts a NaN
    into min and max of its column."""
    big = torch.full((len(table) + 2 * GUARD, D + 2), float("nan"), dtype=torch.float32)
    big[GUARD:-GUARD, :D] = torch.from_numpy(table)
    return big.to(dev)[GUARD:-GUARD, :D]


def check(state, action, ep_end, idx, stride, mirror, *, delta_mask, clip, left=7, right=7, what=""):
    spec = ns.ChunkSpec("s", "a", WIDTH, clip, clip, False, delta_mask)
    s_rows, a_rows = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=WIDTH, clip_state=clip, clip_action=clip,
                                   mask_state=False, delta_mask=delta_mask, frame_idx=idx, frame_stride=stride, frame_mirror=mirror,
                                   left_dim=left, right_dim=right)  # fmt: skip
    res = ns.device_results(state, action, ep_end, spec, HORIZON, idx, frame_stride=stride, frame_mirror=mirror, left_dim=left, right_dim=right)
    for key, rows in (("state", s_rows), ("actions", a_rows)):
        ref, r = refs.Reference(rows), res[key]
        tag = f"{what} {key}"
        assert r.sums.count == ref.n
        ref.check_sums(r.sums.lo, r.sums.hi, r.sums.sum, r.sums.sumsq, tag)
        assert np.array_equal(r.edges, ref.edges), f"{tag}: edges differ"
        diff = np.flatnonzero((r.hist != ref.hist).any(1))
        assert diff.size == 0, f"{tag}: histogram counts differ in columns {diff.tolist()}"
        ref.check_stats(r.stats, tag)
    # the two entry points themselves at the padded width, on tables framed by NaN
    dev = torch.device("cuda")
    t_state, t_action = _guarded(state, dev), _guarded(action, dev)
    assert t_state.stride(0) == D + 2 and not torch.isnan(t_state).any()
    t_end = torch.from_numpy(ep_end.astype(np.int32)).to(dev)
    t_idx = torch.from_numpy(idx.astype(np.int32)).to(dev)
    view = (None if stride is None else torch.from_numpy(stride).to(dev), None if mirror is None else torch.from_numpy(mirror).to(dev), left, right)
    kw = dict(horizon=HORIZON, width=WIDTH, clip_state=clip, clip_action=clip, mask_state=False, delta_mask=delta_mask, view=view)
    sums = ns.device_sums(t_state, t_action, t_end, t_idx, **kw)
    ref.check_sums(sums.lo, sums.hi, sums.sum, sums.sumsq, f"{what} actions, guarded entry points")
    varying = ref.lo != ref.hi
    hist = ns.device_hist(t_state, t_action, t_end, t_idx, ref.edges, sum(1 << int(c) for c in np.flatnonzero(varying)), **kw)
    assert np.array_equal(hist[varying], ref.hist[varying]) and not hist[~varying].any(), f"{what}: guarded histogram differs"
    return res


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("delta_mask", [SYMMETRIC, LEFT_ONLY], ids=["symmetric", "left_only"])
@pytest.mark.parametrize("which", ["small", "large"])
def test_views_against_chunk_rows(tables, which, delta_mask, clip):
    state, action, ep_end = tables[which]
    assert (np.abs(action[:, :7]) > refs.PI32).any() and (np.abs(action[:, 7:]) > refs.PI32).any()
    idx, stride, mirror = _view(len(state), seed=len(state))
    # strides step past episode ends (and, in the last episode, past the table): the clamp is to the last KEPT row
    last = idx + (ep_end[idx] - 1 - idx) // stride * stride
    assert ((idx + (HORIZON - 1) * stride > last).any() and (idx + (HORIZON - 1) * stride >= len(state)).any() and (last < ep_end[idx] - 1).any())
    res = check(state, action, ep_end, idx, stride, mirror, delta_mask=delta_mask, clip=clip, what=f"{which} mask={delta_mask:#x} clip={clip}")
    if not clip:
        assert res["actions"].sums.hi.max() >= 4.0  # nothing filtered
    # the mirror is in play: the same frames unmirrored give other statistics
    plain = ns.device_results(state, action, ep_end, ns.ChunkSpec("s", "a", WIDTH, clip, clip, False, delta_mask), HORIZON, idx, frame_stride=stride)
    assert not np.array_equal(plain["actions"].sums.sum, res["actions"].sums.sum)


def test_one_array_each_uneven_arms_and_any_stride_value(tables):
    """frame_stride alone, frame_mirror alone, arms of 6 + 8 and of 5 + 11 (the whole width: the two zero-padded columns travel with the right arm), and strides the table cannot
    hold (2^31 - 1 next to 1): the row is i + min(h, steps) * stride with steps = (last - i) / stride, so nothing overflows and
    nothing outside the NaN frame is read."""
    state, action, ep_end = tables["small"]
    idx, stride, mirror = _view(len(state), seed=5)
    check(state, action, ep_end, idx, stride, None, delta_mask=SYMMETRIC, clip=True, what="stride only")
    check(state, action, ep_end, idx, None, mirror, delta_mask=LEFT_ONLY, clip=True, what="mirror only")
    check(state, action, ep_end, idx, stride, mirror, delta_mask=LEFT_ONLY, clip=True, left=6, right=8, what="6 + 8")
    check(state, action, ep_end, idx, stride, mirror, delta_mask=SYMMETRIC, clip=False, left=5, right=11, what="5 + 11 = width")
    huge = np.where(np.arange(len(idx)) % 2 == 0, 2**31 - 1, 1).astype(np.int32)
    spec = ns.ChunkSpec("s", "a", WIDTH, True, True, False, SYMMETRIC)
    with pytest.raises(ValueError, match="frame_stride must lie in"):  # the public path refuses it before any upload
        ns.device_results(state, action, ep_end, spec, HORIZON, idx, frame_stride=huge)
    dev = torch.device("cuda")
    kw = dict(horizon=HORIZON, width=WIDTH, clip_state=True, clip_action=True, mask_state=False, delta_mask=SYMMETRIC,
              view=(torch.from_numpy(huge).to(dev), None, 7, 7))  # fmt: skip
    sums = ns.device_sums(_guarded(state, dev), _guarded(action, dev), torch.from_numpy(ep_end).to(dev), torch.from_numpy(idx.astype(np.int32)).to(dev), **kw)
    _, rows = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=WIDTH, clip_state=True, clip_action=True, mask_state=False,
                            delta_mask=SYMMETRIC, frame_idx=idx, frame_stride=huge)  # fmt: skip
    refs.Reference(rows).check_sums(sums.lo, sums.hi, sums.sum, sums.sumsq, "stride 2^31 - 1")


def test_null_views_are_the_existing_entry_points(tables):
    """frame_stride = frame_mirror = NULL: the same launches, the same bits — with and without frame_idx."""
    state, action, ep_end = tables["large"]
    dev = torch.device("cuda")
    t_state, t_action, t_end = (torch.from_numpy(x).to(dev) for x in (state, action, ep_end))
    idx = torch.from_numpy(_view(len(state), seed=3)[0].astype(np.int32)).to(dev)
    kw = dict(horizon=HORIZON, width=WIDTH, clip_state=True, clip_action=True, mask_state=False, delta_mask=SYMMETRIC)
    for t_idx in (None, idx):
        old, new = (ns.device_sums(t_state, t_action, t_end, t_idx, **kw, view=v) for v in (None, (None, None, 7, 7)))
        for f in ("lo", "hi", "sum", "sumsq"):
            assert getattr(old, f).tobytes() == getattr(new, f).tobytes(), f
        edges = np.stack([ns.column_edges(old.lo[c], old.hi[c]) for c in range(WIDTH)])
        mask = sum(1 << c for c in range(WIDTH) if old.lo[c] != old.hi[c])
        h_old, h_new = (ns.device_hist(t_state, t_action, t_end, t_idx, edges, mask, **kw, view=v) for v in (None, (None, None, 7, 7)))
        assert np.array_equal(h_old, h_new) and h_old.sum() == (len(state) if t_idx is None else len(idx)) * HORIZON * bin(mask).count("1")
    # ... and stride 1 everywhere with no frame mirrored, through the view kernels, is the same statistic
    ones = torch.ones(len(idx), dtype=torch.int32, device=dev)
    zeros = torch.zeros(len(idx), dtype=torch.uint8, device=dev)
    same = ns.device_sums(t_state, t_action, t_end, idx, **kw, view=(ones, zeros, 7, 7))
    assert all(getattr(old, f).tobytes() == getattr(same, f).tobytes() for f in ("lo", "hi", "sum", "sumsq"))


def test_refusals_launch_nothing(tables):
    state, action, ep_end = tables["small"]
    dev = torch.device("cuda")
    n = len(state)
    t_state, t_action, t_end = (torch.from_numpy(x).to(dev) for x in (state, action, ep_end))
    stride = torch.ones(n, dtype=torch.int32, device=dev)
    mirror = torch.ones(n, dtype=torch.uint8, device=dev)
    out = torch.full((4, WIDTH), -7.0, dtype=torch.float64, device=dev)
    ws = torch.full((_lib.load().kai0_chunk_stats_workspace_bytes(n, WIDTH) // 8,), -7.0, dtype=torch.float64, device=dev)
    hist = torch.zeros(WIDTH, 100, dtype=torch.int64, device=dev)
    edges = torch.linspace(-4, 4, 101, dtype=torch.float64).repeat(WIDTH, 1).to(dev)
    ok = dict(state=t_state.data_ptr(), ld_state=D, ds=D, action=t_action.data_ptr(), ld_action=D, da=D, ep_end=t_end.data_ptr(), N=n,
              frame_idx=None, frame_stride=stride.data_ptr(), frame_mirror=mirror.data_ptr(), left_dim=7, right_dim=7, M=n, horizon=HORIZON,
              width=WIDTH, clip_state=1, clip_action=1, mask_state=0, delta_mask=SYMMETRIC)  # fmt: skip
    tail_m = (out.data_ptr(), ws.data_ptr(), ws.numel() * 8, None)
    tail_h = (edges.data_ptr(), 100, (1 << D) - 1, hist.data_ptr(), None)
    for change, msg in ((dict(left_dim=9, right_dim=8), "must fit width=16"), (dict(left_dim=-1), "left_dim=-1"), (dict(right_dim=-2), "right_dim=-2"),
                        (dict(ep_end=None), "null buffer"), (dict(action=None), "null buffer"), (dict(frame_stride=stride.data_ptr() + 2), "not aligned"),
                        (dict(horizon=0), "horizon=0"), (dict(width=33), "width=33")):  # fmt: skip
        for name, tail in (("kai0_chunk_stats_moments_view", tail_m), ("kai0_chunk_stats_hist_view", tail_h)):
            with pytest.raises(_lib.Kai0HipError, match=msg):
                _lib.call(name, *{**ok, **change}.values(), *tail)
    with pytest.raises(_lib.Kai0HipError, match="out must be"):
        _lib.call("kai0_chunk_stats_moments_view", *ok.values(), None, ws.data_ptr(), ws.numel() * 8, None)
    with pytest.raises(_lib.Kai0HipError, match="workspace"):
        _lib.call("kai0_chunk_stats_moments_view", *ok.values(), out.data_ptr(), ws.data_ptr(), 8, None)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all()) and not bool(hist.any())  # nothing ran
    spec = ns.ChunkSpec("s", "a", WIDTH, True, True, False, SYMMETRIC)
    with pytest.raises(ValueError, match="do not fit action_dim"):
        ns.device_results(state, action, ep_end, spec, HORIZON, frame_mirror=np.ones(n, np.uint8), left_dim=9, right_dim=8)
    with pytest.raises(ValueError, match="one entry per frame"):
        ns.device_results(state, action, ep_end, spec, HORIZON, frame_stride=np.ones(n + 1, np.int32))
    with pytest.raises(ValueError, match="frame_stride must lie in"):  # stride x horizon must fit int32
        ns.device_results(state, action, ep_end, spec, HORIZON, frame_stride=np.full(n, 2**31 // HORIZON + 1))
    _lib.call("kai0_chunk_stats_moments_view", *ok.values(), *tail_m)  # the accepted call does run
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any())


def test_compute_norm_stats_of_an_augmented_config_equals_the_host_path(tmp_path):
    """space_mirror + TimeScaling(2, 0.3) end to end on a dataset directory: the device path against device="cpu" (what --host runs)
    and against the rows of the plan the loader uses."""
    import dataclasses

    from test_norm_stats_cpu import HORIZON as H
    from test_norm_stats_cpu import _train_config

    lengths = [7, 10, 1]
    state, action, ep_end = _tables(lengths, seed=4)
    root = refs.write_dataset(tmp_path / "FlattenFold", lengths, state, action)
    cfg = _train_config(root, tmp_path / "assets", use_delta_joint_actions=True, space_mirror=True, time_scaling=lrd.TimeScaling(2, 0.3))
    dev, host = ns.compute_norm_stats(cfg), ns.compute_norm_stats(cfg, device="cpu")
    plan = lrd.plan_view(lengths, None, lrd.TimeScaling(2, 0.3), True)
    assert len(plan) == 2 * (4 + 10 + 1) and plan.frame_stride.tolist()[:5] == [2, 2, 2, 2, 1] and plan.frame_mirror.sum() == 15
    s, a = ns.chunk_rows(state, action, ep_end, horizon=H, action_dim=32, clip_state=True, clip_action=True, mask_state=False,
                         delta_mask=SYMMETRIC, frame_idx=plan.frame_idx, frame_stride=plan.frame_stride, frame_mirror=plan.frame_mirror)  # fmt: skip
    for key, rows in (("state", s), ("actions", a)):
        assert np.array_equal(dev[key].q01, host[key].q01) and np.array_equal(dev[key].q99, host[key].q99)
        ref = refs.Reference(rows)
        ref.check_stats(dev[key], f"augmented, device {key}")
        ref.check_stats(host[key], f"augmented, host {key}")
    # the union with the mirror makes the two arms' statistics equal; the plain config's are not
    assert np.array_equal(dev["actions"].q99[:7], dev["actions"].q99[7:14])
    plain = ns.compute_norm_stats(dataclasses.replace(cfg, data=dataclasses.replace(cfg.data, space_mirror=False, time_scaling=None)))
    assert not np.array_equal(plain["actions"].q99[:7], plain["actions"].q99[7:14])
