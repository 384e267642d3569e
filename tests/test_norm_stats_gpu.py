"""Normalisation statistics on the MI355X (csrc/norm_stats.hip through kai0_amd.norm_stats): the device path against the virtual rows
themselves.  Every case builds the rows with `chunk_rows` (held to the real transform stack bit for bit by test_norm_stats_cpu.py),
takes the pinned estimator's one-shot answer and the exact `math.fsum` sums from them (norm_stats_refs.Reference) and compares:
  hist bit for bit as integers, min / max exact, q01 / q99 bit for bit, sum and sum of squares within (n - 1) 2^-53 sum|x| of the
  exact value (the bound of ANY summation order, derived in norm_stats_refs), mean / std through the same bound."""

import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import norm_stats_refs as refs  # noqa: E402
from kai0_amd import norm_stats as ns  # noqa: E402

pytestmark = pytest.mark.gpu

AGILEX_DELTA = 0b01111110111111  # make_bool_mask(6, -1, 6, -1)
EDGE_LENGTHS = [1, 2, 3, 49, 50, 51, 157]  # around the horizon: windows clamped from the first row on, by one row, not at all


def check(state, action, ep_end, *, horizon, width, clip_state=True, clip_action=True, mask_state=False, delta_mask=0, frame_idx=None,
          what=""):  # fmt: skip
    """Both keys through the device path, against the references of the same rows."""
    spec = ns.ChunkSpec("s", "a", width, clip_state, clip_action, mask_state, delta_mask)
    s_rows, a_rows = ns.chunk_rows(state, action, ep_end, horizon=horizon, action_dim=width, clip_state=clip_state, clip_action=clip_action,
                                   mask_state=mask_state, delta_mask=delta_mask, frame_idx=frame_idx)  # fmt: skip
    res = ns.device_results(state, action, ep_end, spec, horizon, frame_idx)
    for key, rows in (("state", s_rows), ("actions", a_rows)):
        ref, r = refs.Reference(rows), res[key]
        tag = f"{what} {key} H={horizon} width={width}"
        assert r.sums.count == ref.n
        ref.check_sums(r.sums.lo, r.sums.hi, r.sums.sum, r.sums.sumsq, tag)
        assert r.hist.dtype == np.int64 and np.array_equal(r.edges, ref.edges), f"{tag}: edges differ"
        diff = np.flatnonzero((r.hist != ref.hist).any(1))
        assert diff.size == 0, f"{tag}: histogram counts differ in columns {diff.tolist()}"
        if ref.stats is not None:
            ref.check_stats(r.stats, tag)
    # the public path launches only the columns that can be non-zero; the two entry points themselves at the full, padded width
    dev = torch.device("cuda")
    t_state, t_action = torch.from_numpy(state).to(dev), torch.from_numpy(action).to(dev)
    t_end = torch.from_numpy(ep_end.astype(np.int32)).to(dev)
    t_idx = None if frame_idx is None else torch.from_numpy(np.asarray(frame_idx, np.int32)).to(dev)
    kw = dict(horizon=horizon, width=width, clip_state=clip_state, clip_action=clip_action, mask_state=mask_state, delta_mask=delta_mask)
    sums = ns.device_sums(t_state, t_action, t_end, t_idx, **kw)
    ref.check_sums(sums.lo, sums.hi, sums.sum, sums.sumsq, f"{what} actions, entry points at width={width}")
    varying = ref.lo != ref.hi
    if varying.any():
        hist = ns.device_hist(t_state, t_action, t_end, t_idx, ref.edges, sum(1 << int(c) for c in np.flatnonzero(varying)), **kw)
        assert np.array_equal(hist[varying], ref.hist[varying]) and not hist[~varying].any(), f"{what}: padded-width histogram differs"
    return res


@pytest.fixture(scope="module")
def edge_tables():
    out = {}
    for d in (14, 7):
        state, action, ep_end = refs.random_walk_table(EDGE_LENGTHS, ds=d, da=d, seed=d, grippers=(6, 13), scale=0.3)
        out[d] = (*refs.boundary_values(state, action), ep_end)
    return out


@pytest.mark.parametrize("horizon", [50, 4, 1])
@pytest.mark.parametrize("d, width", [(14, 32), (7, 8)])
def test_clamp_edges(edge_tables, horizon, d, width):
    """Episodes of 1, 2, 3, 49, 50, 51 and 157 frames (N = 313): at H = 50 every window of the first five is clamped; tables of
    14 and 7 columns padded to 32 and 8."""
    state, action, ep_end = edge_tables[d]
    check(state, action, ep_end, horizon=horizon, width=width, delta_mask=AGILEX_DELTA & ((1 << d) - 1), what="clamp")


@pytest.mark.parametrize("delta, clip_state, mask_state", [(True, True, False), (False, True, False), (True, False, False),
                                                           (False, False, False), (True, True, True)])  # fmt: skip
def test_transforms(edge_tables, delta, clip_state, mask_state):
    """Delta mask (6, -1, 6, -1) on / off, the state filter on / off (ARX), a masked state; both tables hold +-f32(pi) (kept), the
    next f32 beyond it and a 4.0 glitch (dropped), -0.0."""
    state, action, ep_end = edge_tables[14]
    assert (np.abs(action) == refs.PI32).any() and (np.abs(action) > refs.PI32).sum() >= 4 and (np.abs(state) > refs.PI32).sum() >= 4
    res = check(state, action, ep_end, horizon=4, width=32, clip_state=clip_state, mask_state=mask_state,
                delta_mask=AGILEX_DELTA if delta else 0, what=f"delta={delta} clip_state={clip_state} mask_state={mask_state}")  # fmt: skip
    if not delta:
        assert res["actions"].sums.hi.max() == float(refs.PI32)  # f32(pi) itself survives the filter
    if not clip_state and not mask_state:
        assert res["state"].sums.hi.max() >= 4.0  # nothing filtered: the glitch (and the walk beyond pi) is in the statistic


def test_many_blocks():
    """N = 12 000 frames x H = 50 in 14 columns: 600 k virtual rows.  At this N neither grid is capped (pass 1: 375 blocks of 8
    frames per trip, pass 2: 24 blocks x 2 column groups of 128 frames per trip), and every block walks its grid-stride loop 4
    times — the same loop a capped grid runs longer."""
    lengths = [300] * 39 + [157, 143]
    assert sum(lengths) == 12_000
    state, action, ep_end = refs.random_walk_table(lengths, seed=5)
    check(state, action, ep_end, horizon=50, width=14, delta_mask=AGILEX_DELTA, what="many blocks")


def test_concentration():
    """Same-address pressure on the LDS counters: a column where all but 3 virtual rows share one value (the 3 odd values sit on
    first frames of episodes, which no earlier window reaches), a two-valued column, a column spanning 1e-6 .. 3 log-uniformly."""
    lengths = [200] * 10
    state, action, ep_end = refs.random_walk_table(lengths, seed=9)
    rng = np.random.default_rng(9)
    action[:, 0] = 0.25
    action[[0, 200, 1800], 0] = [0.5, -0.75, 0.26]
    action[:, 1] = np.where(rng.random(2000) < 0.9, 0.0, 0.07)
    action[:, 2] = np.exp(rng.uniform(np.log(1e-6), np.log(3.0), 2000))
    action[:2, 2] = [1e-6, 3.0]
    res = check(state, action, ep_end, horizon=50, width=14, delta_mask=0, what="concentration")
    h = res["actions"].hist
    assert np.sort(h[0][h[0] > 0]).tolist() == [1, 1, 1, 2000 * 50 - 3] and (h[1] > 0).sum() == 2


def test_subsets():
    """frame_idx unsorted and with duplicates, a single frame, and a permutation of all N."""
    state, action, ep_end = refs.random_walk_table([1, 30, 77, 2, 51], seed=2)
    n = len(state)
    rng = np.random.default_rng(0)
    for idx in (rng.integers(0, n, size=97), np.array([0, 0, n - 1, n - 1, 31, 31, 31]), np.array([108]), rng.permutation(n)):
        check(state, action, ep_end, horizon=50, width=32, delta_mask=AGILEX_DELTA, frame_idx=idx, what=f"subset M={len(idx)}")
    whole = ns.device_results(state, action, ep_end, ns.ChunkSpec("s", "a", 32, True, True, False, AGILEX_DELTA), 50)
    perm = ns.device_results(state, action, ep_end, ns.ChunkSpec("s", "a", 32, True, True, False, AGILEX_DELTA), 50, rng.permutation(n))
    assert np.array_equal(whole["actions"].hist, perm["actions"].hist)  # integer counts do not depend on the order
    with pytest.raises(ValueError, match="frame_idx outside the table"):
        ns.device_results(state, action, ep_end, ns.ChunkSpec("s", "a", 32, True, True, False, 0), 50, np.array([n]))


def test_non_finite_values_are_refused():
    state, action, ep_end = refs.random_walk_table([40, 40], seed=4)
    spec = ns.ChunkSpec("s", "a", 32, True, True, False, AGILEX_DELTA)
    action[55, 9] = np.nan
    with pytest.raises(ValueError, match=r"key 'actions', column 9 "):
        ns.device_results(state, action, ep_end, spec, 50)
    action[55, 9] = 0.0
    state[3, 2] = np.inf  # the glitch filter removes an infinity ...
    ns.device_results(state, action, ep_end, spec, 50)
    with pytest.raises(ValueError, match=r"key 'state', column 2 "):  # ... unless the robot has none (ARX)
        ns.device_results(state, action, ep_end, ns.ChunkSpec("s", "a", 32, False, True, False, 0), 50)


def test_compute_norm_stats_equals_the_host_path(tmp_path):
    """End to end on a dataset directory: parquet columns -> device -> NormStats against `device="cpu"` (what --host runs):
    histogram-derived fields equal, mean / std within the summation bound."""
    from test_norm_stats_cpu import HORIZON, _train_config

    lengths = [1, 2, 5, 9, 33]
    state, action, ep_end = refs.random_walk_table(lengths, seed=3, scale=0.4)
    refs.boundary_values(state, action)
    root = refs.write_dataset(tmp_path / "FlattenFold", lengths, state, action)
    cfg = _train_config(root, tmp_path / "assets", use_delta_joint_actions=True)
    dev, host = ns.compute_norm_stats(cfg), ns.compute_norm_stats(cfg, device="cpu")
    s, a = ns.chunk_rows(state, action, ep_end, horizon=HORIZON, action_dim=32, clip_state=True, clip_action=True, mask_state=False,
                         delta_mask=AGILEX_DELTA)  # fmt: skip
    for key, rows in (("state", s), ("actions", a)):
        assert np.array_equal(dev[key].q01, host[key].q01) and np.array_equal(dev[key].q99, host[key].q99)
        ref = refs.Reference(rows)
        ref.check_stats(dev[key], f"end to end {key}")
        ref.check_stats(host[key], f"end to end (host) {key}")
    sub_dev, sub_host = ns.compute_norm_stats(cfg, max_frames=20, seed=1), ns.compute_norm_stats(cfg, max_frames=20, seed=1, device="cpu")
    assert np.array_equal(sub_dev["actions"].q99, sub_host["actions"].q99) and not np.array_equal(sub_dev["actions"].q99, dev["actions"].q99)
    assert torch.cuda.is_available()
