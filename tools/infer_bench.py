"""p50 of one B = 1 action chunk + stage split, without the training bench (quick iteration on the inference path).
usage: python tools/infer_bench.py [--pi0]      (--pi0: Pi0Config(pi05=False) — 48 prompt slots, a state token; adds the time of the
ten steps' suffix-embedding launches, ops.pi0_suffix_embed, replayed from a graph of their own)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from kai0_amd.config import Pi0Config  # noqa: E402

dev = torch.device("cuda:0")
pi0 = "--pi0" in sys.argv[1:]
cfg = Pi0Config(pi05=not pi0)
model = bench.build_model(cfg, dev, 0)
res = bench.measure_latency(model, cfg, dev, iters=40)
res["model_type"] = cfg.model_type
if pi0:
    from kai0_amd import ops
    from kai0_amd.infer import euler_times

    model.trim_prompt_padding_infer = False
    obs, _ = bench.synthetic_batch(cfg, 1, seed=123, device=dev)
    model.sample_actions(dev, obs, noise=torch.randn(1, cfg.action_horizon, cfg.action_dim, device=dev), num_steps=10)
    eng = model._engine
    res["engine_fast"] = bool(eng.fast)
    tvec, _ = eng._time_vectors(euler_times(10))
    Hs, Ss, De = eng.Hs, eng.Ss, eng.De
    x2 = torch.randn(Hs, cfg.action_dim, device=dev)
    xs = torch.empty((Ss, De), dtype=torch.bfloat16, device=dev)
    sq = torch.zeros((De // 16, Ss), dtype=torch.float32, device=dev)

    def ten():
        for step in range(10):
            ops.pi0_suffix_embed(x2, model.action_in_proj.weight, model.action_in_proj.bias, model.action_time_mlp_in.weight, tvec[step],
                                 model.action_time_mlp_out.weight, model.action_time_mlp_out.bias, xs, sq, Hs, Ss)

    res["suffix_embed_10_steps_ms"] = bench._graph_time_ms(ten)
print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))
