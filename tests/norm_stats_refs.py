"""Synthetic tables, exact sums and the summation bound for the normalisation-statistics tests (kai0_amd/norm_stats.py,
csrc/norm_stats.hip).  A plain helper module like tests/streaming_refs.py: nothing here touches the HIP library.

  * `random_walk_table` / `write_dataset` — episodes of joint-like random walks (two gripper-like columns on two values) as the
    two f32 tables + ep_end, and the same thing as a LeRobot v2 directory with state / action columns only (no camera feature).
  * `Reference`  — what the tests hold a result to, from the virtual rows themselves: the pinned estimator in its one-shot form
    (`RunningStats().update(rows.astype(float64))`: integer counts, edges, q01 / q99, mean / std), exact min / max, and the EXACT sum
    and sum of squares by `math.fsum` (the square of an f32 value is exact in f64, so the list of squares is exact too).
  * `sum_bound`  — |computed - exact| <= (n - 1) 2^-53 sum|x| for a sum of n f64 addends in ANY order (every one of the n - 1
    additions rounds a partial sum whose magnitude is at most sum|x|, to first order in 2^-53; Higham, Accuracy and Stability of
    Numerical Algorithms, §4.2).  Derived, not measured; `mean_bound` / `std_bound` carry it through the two formulas."""

import json
import math

import numpy as np

from kai0_amd.normalize import RunningStats

U = 2.0**-53
PI32 = np.float32(np.pi)
FPS = 30


def random_walk_table(lengths, ds=14, da=14, seed=0, grippers=(6, 13), scale=0.02):
    """state f32 [N, ds], action f32 [N, da], ep_end int32 [N]: per episode a random walk of joint angles around [-1.5, 1.5]; the
    action is the state one step ahead plus noise; the gripper columns sit on the two values 0 / 0.07."""
    rng = np.random.default_rng(seed)
    states, actions = [], []
    for n in lengths:
        w = max(ds, da)
        walk = rng.uniform(-1.5, 1.5, size=(1, w)) + np.cumsum(rng.normal(0, scale, size=(n + 1, w)), axis=0)
        for g in grippers:
            if g < w:
                walk[:, g] = np.where(np.sin(np.arange(n + 1) / 7.0 + g) > 0, 0.07, 0.0)
        states.append(walk[:n, :ds])
        act = walk[1:, :da] + rng.normal(0, scale / 10, size=(n, da))
        for g in grippers:
            if g < da:
                act[:, g] = walk[1:, g]
        actions.append(act)
    ends = np.cumsum(lengths)
    return (np.concatenate(states).astype(np.float32), np.concatenate(actions).astype(np.float32),
            np.repeat(ends, lengths).astype(np.int32))  # fmt: skip


def boundary_values(state, action):
    """Plant the glitch-filter boundary in both tables (in place): +-f32(pi) (kept), the next f32 above it (dropped), a 4.0 glitch,
    -0.0."""
    vals = np.array([PI32, -PI32, np.nextafter(PI32, np.float32(np.inf)), -np.nextafter(PI32, np.float32(np.inf)), 4.0, -4.0, -0.0],
                    np.float32)  # fmt: skip
    for t, shift in ((state, 0), (action, 3)):
        n, d = t.shape
        for k, v in enumerate(vals):
            t[(k * 5 + shift) % n, (k * 3 + shift) % d] = v
            t[(n - 1 - k - shift) % n, (k + shift) % d] = v
    return state, action


def write_dataset(root, lengths, state, action):
    """A LeRobot v2 directory holding the two vector columns and the scalar index columns only — no image or video feature."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    root.mkdir(parents=True, exist_ok=True)
    (root / "meta").mkdir(exist_ok=True)
    feats = {"observation.state": {"dtype": "float32", "shape": [state.shape[1]]}, "action": {"dtype": "float32", "shape": [action.shape[1]]},
             "timestamp": {"dtype": "float32", "shape": [1]}, "frame_index": {"dtype": "int64", "shape": [1]},
             "episode_index": {"dtype": "int64", "shape": [1]}, "index": {"dtype": "int64", "shape": [1]},
             "task_index": {"dtype": "int64", "shape": [1]}}  # fmt: skip
    info = {"codebase_version": "v2.1", "fps": FPS, "chunks_size": 1000, "total_episodes": len(lengths), "features": feats,
            "data_path": "data/chunk-{episode_chunk:03d}/episode_{episode_index:06d}.parquet",
            "video_path": "videos/chunk-{episode_chunk:03d}/{video_key}/episode_{episode_index:06d}.mp4"}  # fmt: skip
    (root / "meta" / "info.json").write_text(json.dumps(info))
    (root / "meta" / "tasks.jsonl").write_text(json.dumps({"task_index": 0, "task": "Flatten and fold the cloth."}))
    (root / "meta" / "episodes.jsonl").write_text(
        "\n".join(json.dumps({"episode_index": e, "tasks": ["Flatten and fold the cloth."], "length": int(n)}) for e, n in enumerate(lengths)))
    g = 0
    for e, n in enumerate(lengths):
        arrays = {"observation.state": pa.array(list(state[g : g + n]), type=pa.list_(pa.float32())),
                  "action": pa.array(list(action[g : g + n]), type=pa.list_(pa.float32())),
                  "timestamp": pa.array(np.arange(n, dtype=np.float32) / FPS), "frame_index": pa.array(np.arange(n)),
                  "episode_index": pa.array(np.full(n, e)), "index": pa.array(np.arange(g, g + n)),
                  "task_index": pa.array(np.zeros(n, np.int64))}  # fmt: skip
        p = root / f"data/chunk-000/episode_{e:06d}.parquet"
        p.parent.mkdir(parents=True, exist_ok=True)
        pq.write_table(pa.table(arrays), p)
        g += n
    return root


def sum_bound(n: int, abs_sum: float) -> float:
    return (n - 1) * U * abs_sum


class Reference:
    """Everything a result is compared with, from the f32 rows [..., D] (computed once per table; never modified)."""

    def __init__(self, rows: np.ndarray):
        x = np.asarray(rows, np.float32).reshape(-1, np.shape(rows)[-1]).astype(np.float64)
        self.n, self.d = x.shape
        self.lo, self.hi = x.min(0), x.max(0)
        self.sum = np.array([math.fsum(x[:, c]) for c in range(self.d)])
        self.sumsq = np.array([math.fsum(x[:, c] * x[:, c]) for c in range(self.d)])
        self.abs_sum = np.array([math.fsum(np.abs(x[:, c])) for c in range(self.d)])
        self.sum_bound = np.array([sum_bound(self.n, a) for a in self.abs_sum])
        self.sumsq_bound = np.array([sum_bound(self.n, a) for a in self.sumsq])  # the squares are their own absolute values
        rs = RunningStats()
        rs.update(x)
        self.stats = rs.get_statistics() if self.n >= 2 else None  # (the estimator refuses a single row)
        self.hist = np.stack(rs.hist).astype(np.int64)
        assert np.array_equal(self.hist, np.stack(rs.hist)) and self.hist.sum(1).tolist() == [self.n] * self.d
        self.edges = np.stack(rs.edges)
        # mean = S1 / n and var = S2 / n - mean^2 from the exact sums; one rounding each for the divisions, the square and the difference
        self.mean = self.sum / self.n
        m2 = self.sumsq / self.n
        self.std = np.sqrt(np.maximum(0, m2 - self.mean**2))
        self.mean_bound = self.sum_bound / self.n + 2 * U * np.abs(self.mean)
        # |var' - var| <= dS2 / n + (2 |mean| + dmean) dmean, plus the final roundings of both sides (4 operations each, on magnitudes
        # <= m2 + mean^2); |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|)
        dvar = self.sumsq_bound / self.n + (2 * np.abs(self.mean) + self.mean_bound) * self.mean_bound + 16 * U * (m2 + self.mean**2)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.std_bound = np.minimum(np.where(self.std > 0, dvar / self.std, np.inf), np.sqrt(dvar)) + 2 * U * self.std

    def check_sums(self, lo, hi, s1, s2, what=""):
        assert np.array_equal(lo, self.lo) and np.array_equal(hi, self.hi), f"{what}: min / max differ"
        e1, e2 = np.abs(s1 - self.sum), np.abs(s2 - self.sumsq)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(np.nanmax(np.where(self.sum_bound > 0, e1 / self.sum_bound, 0)), np.nanmax(np.where(self.sumsq_bound > 0, e2 / self.sumsq_bound, 0)))
        print(f"{what}: n={self.n} worst sum error / bound {worst:.3e}")
        assert np.all(e1 <= self.sum_bound) and np.all(e2 <= self.sumsq_bound), f"{what}: sum error {e1.max():.3e} / {e2.max():.3e} outside the bound"

    def check_stats(self, st, what="", exact_hist_fields=True):
        if exact_hist_fields:
            assert np.array_equal(st.q01, self.stats.q01) and np.array_equal(st.q99, self.stats.q99), f"{what}: q01 / q99 differ"
        em, es = np.abs(st.mean - self.mean), np.abs(st.std - self.std)
        assert np.all(em <= self.mean_bound), f"{what}: mean off by {em.max():.3e}"
        assert np.all(es <= self.std_bound), f"{what}: std off by {(es - self.std_bound).max():.3e} beyond its bound"
