"""Golden results for space mirroring, produced by EXECUTING THE REFERENCE'S OWN CODE in the build container (needs the reference
checkout that tests/reflift.py points to; nothing is imported from it and nothing of it is copied — its source is read and compiled
when this script runs):

  * `swap_arms_in_array`, `swap_array_dims_list`, `swap_stats_dims` and `process_norm_stats_json`
    (train_deploy_alignment/data_augment/space_mirroring.py) are lifted with tests/reflift.py and run on seeded inputs: parquet-cell
    rows of 7 + 7 and 6 + 8 values, a wrong-length row (its ValueError message is recorded), norm-stats lists of 14 and of 32 entries
    (padding after the arms), a per-episode stats dictionary, and a norm_stats.json written to and read back from a temporary
    directory.

    python tests/golden/make_data_augment_golden.py   ->  tests/golden/data_augment.npz, tests/golden/data_augment.json
                                                           (inputs and results only)

The time-scaling arithmetic of time_scaling.py sits inside functions that import `lerobot`, which cannot be executed here; the tests
pin it by literal cases derived from the cited lines instead (tests/test_data_augment_cpu.py)."""
import json
import os
import sys
import tempfile
import typing
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import reflift  # noqa: E402

MIRROR_PY = f"{reflift.REF.split('/src/')[0]}/train_deploy_alignment/data_augment/space_mirroring.py"

ns = {"np": np, "json": json, "Path": Path, **{k: getattr(typing, k) for k in ("List", "Tuple", "Dict", "Any", "Optional")}}
reflift.lift(MIRROR_PY, ["swap_arms_in_array", "swap_array_dims_list", "swap_stats_dims", "process_norm_stats_json"], ns)

rng = np.random.default_rng(20261021)
NPZ, JS = {}, {}

# ---- parquet cells ------------------------------------------------------------------------------------------------------------------
rows = rng.normal(size=(5, 14)).astype(np.float32)
NPZ["rows"] = rows
NPZ["rows_swapped_7_7"] = np.stack([ns["swap_arms_in_array"](r) for r in rows])
NPZ["rows_swapped_6_8"] = np.stack([ns["swap_arms_in_array"](r, 6, 8) for r in rows])
try:
    ns["swap_arms_in_array"](rng.normal(size=16).astype(np.float32))
    raise SystemExit("the reference accepted a 16-value row")
except ValueError as e:
    JS["wrong_length_error"] = str(e)

# ---- norm-stats lists: the padding after the arms stays ------------------------------------------------------------------------------
for name, n in (("list14", 14), ("list32", 32)):
    values = rng.normal(size=n).tolist()
    JS[name] = values
    JS[name + "_swapped"] = ns["swap_array_dims_list"](list(values), 7, 7, keep_padding=True)
JS["list32_swapped_5_9"] = ns["swap_array_dims_list"](list(JS["list32"]), 5, 9, keep_padding=True)
try:
    ns["swap_array_dims_list"](rng.normal(size=10).tolist())
    raise SystemExit("the reference accepted a 10-value list")
except ValueError as e:
    JS["short_list_error"] = str(e)

# ---- a norm_stats.json through process_norm_stats_json -------------------------------------------------------------------------------
stats = {"norm_stats": {key: {f: rng.normal(size=32).tolist() for f in ("mean", "std", "q01", "q99")} for key in ("state", "actions")}}
stats["norm_stats"]["extra"] = {"mean": rng.normal(size=3).tolist(), "std": rng.normal(size=3).tolist(), "q01": None, "q99": None}
JS["norm_stats_in"] = json.loads(json.dumps(stats))
with tempfile.TemporaryDirectory() as tmp:
    src, dst = Path(tmp) / "in" / "norm_stats.json", Path(tmp) / "out" / "norm_stats.json"
    src.parent.mkdir()
    src.write_text(json.dumps(stats))
    _, ok, message = ns["process_norm_stats_json"](src, dst)
    assert ok, message
    JS["norm_stats_out"] = json.loads(dst.read_text())

# ---- per-episode statistics: the two hand cameras trade places, state / action lists are swapped ----------------------------------------
ep_stats = {f"observation.images.{cam}": {"mean": rng.uniform(size=3).tolist()} for cam in ("top_head", "hand_left", "hand_right")}
for key in ("observation.state", "action"):
    ep_stats[key] = {f: rng.normal(size=14).tolist() for f in ("min", "max", "mean", "std")}
JS["episode_stats_in"] = json.loads(json.dumps(ep_stats))
JS["episode_stats_out"] = ns["swap_stats_dims"](json.loads(json.dumps(ep_stats)))

np.savez(os.path.join(HERE, "data_augment.npz"), **NPZ)
with open(os.path.join(HERE, "data_augment.json"), "w") as f:
    json.dump(JS, f, indent=1)
print("wrote data_augment.npz", {k: v.shape for k, v in NPZ.items()}, "and data_augment.json", sorted(JS))
