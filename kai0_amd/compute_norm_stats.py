"""`python -m kai0_amd.compute_norm_stats <config-name> [--max-frames N] [--host]` — write the dataset's `norm_stats.json` where
`DataConfigFactory._load_norm_stats` reads it (scripts/compute_norm_stats.py:89-113 of the reference; `kai0_amd.norm_stats`)."""

from __future__ import annotations

import argparse
import logging
from collections.abc import Sequence

from . import norm_stats
from .training_config import get_config


def main(argv: Sequence[str] | None = None):
    ap = argparse.ArgumentParser(description="Compute normalisation statistics for a training config")
    ap.add_argument("config_name")
    ap.add_argument("--max-frames", "--max_frames", dest="max_frames", type=int, default=None,
                    help="use a seeded sample of this many frames")  # fmt: skip
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="compute on the host even if a GPU is present")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    config = get_config(args.config_name)
    stats = norm_stats.compute_norm_stats(config, max_frames=args.max_frames, seed=args.seed, device="cpu" if args.host else None)
    path = norm_stats.save(config, stats)
    print(f"Writing stats to: {path}")
    return path


if __name__ == "__main__":
    main()
