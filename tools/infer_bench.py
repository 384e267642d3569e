"""p50 of one B = 1 action chunk + stage split, without the training bench (quick iteration on the inference path).
usage: python tools/infer_bench.py [--pi0]      (--pi0: Pi0Config(pi05=False) — 48 prompt slots, a state token; adds the time of the
ten steps' suffix-embedding launches, ops.pi0_suffix_embed, replayed from a graph of their own)
       python tools/infer_bench.py --rtc [--pi0]  (adds the p50 of a GUIDED B = 1 chunk — real-time chunking, d = 3, exec_h = 8, "exp",
the previous chunk as 14-dim rows — measured the same way as the unguided p50 beside it, of the same chunk with `mask_prefix_delay`,
and of the same chunk on eager launches; with --pi0 for the state-token model)"""
import time
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
    tvec = eng._schedule(euler_times(10)).tvec
    Hs, Ss, De = eng.Hs, eng.Ss, eng.De
    x2 = torch.randn(Hs, cfg.action_dim, device=dev)
    xs = torch.empty((Ss, De), dtype=torch.bfloat16, device=dev)
    sq = torch.zeros((De // 16, Ss), dtype=torch.float32, device=dev)

    def ten():
        for step in range(10):
            ops.pi0_suffix_embed(x2, model.action_in_proj.weight, model.action_in_proj.bias, model.action_time_mlp_in.weight, tvec[step],
                                 model.action_time_mlp_out.weight, model.action_time_mlp_out.bias, xs, sq, Hs, Ss)

    res["suffix_embed_10_steps_ms"] = bench._graph_time_ms(ten)
if "--rtc" in sys.argv[1:]:
    model.trim_prompt_padding_infer = False
    obs, _ = bench.synthetic_batch(cfg, 1, seed=123, device=dev)
    noise = torch.randn(1, cfg.action_horizon, cfg.action_dim, device=dev)
    prev = torch.randn(cfg.action_horizon, 14).tolist()
    kw0 = dict(prev_action_chunk=prev, inference_delay=3, execute_horizon=8)

    def p50(iters=20, **more):
        kw = {**kw0, **more}
        for _ in range(2):
            model.sample_actions(dev, obs, noise=noise, num_steps=10, **kw)
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            model.sample_actions(dev, obs, noise=noise, num_steps=10, **kw).cpu()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return {"p50_ms": ts[len(ts) // 2], "min_ms": ts[0], "p90_ms": ts[int(len(ts) * 0.9)]}

    rtc = {"captured": p50()}
    eng = model._engine
    rtc["graph"] = eng._g_graph is not None
    rtc["captured_mask_prefix_delay"] = p50(mask_prefix_delay=True)
    eng.use_graph = False
    rtc["eager"] = p50(5)
    eng.use_graph = True
    res["rtc_guided"] = {k: ({a: round(b, 3) for a, b in v.items()} if isinstance(v, dict) else v) for k, v in rtc.items()}
print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))
