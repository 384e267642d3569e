"""Golden results for Stage-Advantage annotation, produced by EXECUTING THE REFERENCE'S OWN CODE in the build container (needs the
reference checkout that tests/reflift.py points to; nothing is imported from it and nothing of it is copied — its source is read and
compiled when this script runs):

  * `SimpleValueEvaluator.evaluate_video_2timesteps_advantages`, `.evaluate_video_1timestep_advantage`, `._process_single_image` and
    `._batch_numpy_to_tensor_parallel` (stage_advantage/annotation/evaluator.py) and `resize_with_pad_torch`
    (shared/image_tools.py) are lifted with tests/reflift.py and run against stubs: `_load_videos_parallel` returns seeded uint8 frames (9 frames, 3 cameras, 24x32), the thread pool is a real one,
    the tokenizer returns fixed ids, and `model.sample_values` is `stage_advantage_refs.stub_sample_values` — a fixed seeded projection
    of the six (or three) images it receives, through tanh.  relative_interval = 3, batch_size = 4: the episode has full-interval
    frames, clamped futures and the last frame whose future is itself.
  * `discretize_advantage.py`'s `main` with its helpers is lifted and run on a small temporary dataset (binary / n_slices, with and
    without stages); the `task_index` columns it writes are the expected values.

    python tests/golden/make_stage_advantage_golden.py   ->  tests/golden/stage_advantage.npz   (frames and result lists only)

tests/test_stage_advantage_cpu.py rebuilds the same observations from `plan_episode`'s tables and the frame restatement and replays the
table through `kai0_amd.stage_advantage.discretize`."""
import logging
import os
import sys
import tempfile
import typing
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reflift  # noqa: E402
import stage_advantage_refs as refs  # noqa: E402

REF_ROOT = reflift.REF.split("/src/")[0]
EVALUATOR_PY = f"{REF_ROOT}/stage_advantage/annotation/evaluator.py"
DISCRETIZE_PY = f"{REF_ROOT}/stage_advantage/annotation/discretize_advantage.py"
IMAGE_TOOLS_PY = f"{REF_ROOT}/src/openpi/shared/image_tools.py"

NUM_FRAMES, H0, W0 = 9, 24, 32
RELATIVE_INTERVAL, BATCH_SIZE = 3, 4
OUT = {}


def typing_ns():
    return {k: getattr(typing, k) for k in ("List", "Tuple", "Dict", "Any", "Optional", "Callable")}


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(20251019)
frames = rng.integers(0, 256, size=(3, NUM_FRAMES, H0, W0, 3), dtype=np.uint8)  # (top, left, right)
OUT["frames"] = frames

tools_ns = {"torch": torch, "F": F}
reflift.lift(IMAGE_TOOLS_PY, ["resize_with_pad_torch"], tools_ns)
ns = {"torch": torch, "np": np, "logging": logging, "SimpleNamespace": SimpleNamespace, "tqdm": lambda it, **kw: it,
      "image_tools": SimpleNamespace(resize_with_pad_torch=tools_ns["resize_with_pad_torch"]), **typing_ns()}  # fmt: skip


class StubEvaluator:
    def __init__(self):
        self.num_workers = 4
        self.device = torch.device("cpu")
        self._executor = ThreadPoolExecutor(max_workers=4)
        self.tokenizer = SimpleNamespace(tokenize=lambda prompt, state=None: (np.arange(1, 9), np.arange(8) < 5))
        self.model = SimpleNamespace(sample_values=refs.stub_sample_values)

    def _load_videos_parallel(self, video_paths, frame_interval=1):
        return tuple([f for f in frames[c]] for c in range(3))


for name in ("_process_single_image", "_batch_numpy_to_tensor_parallel", "evaluate_video_2timesteps_advantages", "evaluate_video_1timestep_advantage"):
    setattr(StubEvaluator, name, reflift.lift_method(EVALUATOR_PY, "SimpleValueEvaluator", name, ns))

ev = StubEvaluator()
kw = dict(video_paths=("top", "left", "right"), prompt="Flatten and fold the cloth.", batch_size=BATCH_SIZE, frame_interval=1,
          relative_interval=RELATIVE_INTERVAL, min_frame_index=0, max_frame_index=NUM_FRAMES - 1)  # fmt: skip
for tag, fn in (("two", ev.evaluate_video_2timesteps_advantages), ("one", ev.evaluate_video_1timestep_advantage)):
    for prefetch in (True, False):
        results = fn(prefetch=prefetch, **kw)
        cols = {k: np.asarray([r[k] for r in results]) for k in results[0]}
        if prefetch:
            for k, v in cols.items():
                OUT[f"{tag}.{k}"] = v
        else:  # the reference's prefetch is a scheduling choice only
            assert all(np.array_equal(OUT[f"{tag}.{k}"], v) for k, v in cols.items())
ev._executor.shutdown()
OUT["relative_interval"], OUT["batch_size"] = np.asarray(RELATIVE_INTERVAL), np.asarray(BATCH_SIZE)

# ---- discretize_advantage.py --------------------------------------------------------------------------------------------------------
import glob  # noqa: E402
import json  # noqa: E402

import pandas as pd  # noqa: E402

dns = {"np": np, "pd": pd, "os": os, "glob": glob, "json": json, "argparse": __import__("argparse"), "tqdm": lambda it, **kw: it,
       **typing_ns()}  # fmt: skip
reflift.lift(DISCRETIZE_PY, ["calculate_rewards", "get_stage_index", "collect_all_rewards", "compute_reward_statistics",
                             "update_tasks_jsonl", "assign_task_index", "assign_task_index_staged", "main"], dns)  # fmt: skip
drng = np.random.default_rng(7)
episodes = []
for n in (23, 17):
    episodes.append({
        "absolute_advantage": np.clip(drng.normal(0.05, 0.4, n), -1, 1),
        "relative_advantage": np.clip(drng.normal(0.0, 0.5, n), -1, 1),
        "stage_progress_gt": np.concatenate([np.sort(drng.uniform(0, 1, n - 2)), [1.0, 0.5]]),
    })  # fmt: skip
OUT["disc.lengths"] = np.asarray([len(e["absolute_advantage"]) for e in episodes])
for k in episodes[0]:
    OUT[f"disc.{k}"] = np.concatenate([e[k] for e in episodes])
OUT["disc.stage_index_3"] = np.asarray([dns["get_stage_index"](s, 3) for s in OUT["disc.stage_progress_gt"]])

CASES = {
    "binary": ["--threshold", "30", "--discretion-type", "binary"],
    "binary_rel_staged2": ["--threshold", "40", "--discretion-type", "binary", "--advantage-source", "relative_advantage", "--stage-nums", "2"],
    "slices5": ["--discretion-type", "n_slices", "--n-slices", "5"],
    "slices4_staged3": ["--discretion-type", "n_slices", "--n-slices", "4", "--stage-nums", "3"],
}  # fmt: skip
for case, argv in CASES.items():
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(f"{tmp}/data/chunk-000")
        for i, e in enumerate(episodes):
            pd.DataFrame({"frame_index": np.arange(len(e["absolute_advantage"])), **e}).to_parquet(f"{tmp}/data/chunk-000/episode_{i:06d}.parquet")
        sys.argv = ["discretize_advantage.py", tmp, *argv]
        dns["main"]()
        OUT[f"disc.{case}.task_index"] = np.concatenate([pd.read_parquet(f)["task_index"].values for f in sorted(glob.glob(f"{tmp}/data/chunk-000/*.parquet"))])
        OUT[f"disc.{case}.tasks"] = np.asarray([json.loads(line)["task"] for line in open(f"{tmp}/meta/tasks.jsonl")])
    OUT[f"disc.{case}.argv"] = np.asarray(argv)

path = os.path.join(HERE, "stage_advantage.npz")
np.savez_compressed(path, **OUT)
print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in OUT.items()})
