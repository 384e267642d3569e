"""kai0_amd.data_loader: host-side loader semantics against the batches of the reference's TorchDataLoader
EXECUTED from source (lifted with `ast`; stubs for jax.tree.map / jax.process_count; recorded in
tests/golden/data_loader_reference.npz by this file when run as a script next to a checkout of the reference), the per-rank sharding under gloo world_size 2, the fake
dataset's shapes, and the device feeder's ordering (CPU device here; the HIP-stream path runs in tests/test_fullsize_gpu.py)."""
import ast
import multiprocessing
import os
import socket
import sys
import types
import typing

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kai0_amd import data_loader as dl  # noqa: E402
from kai0_amd import transforms  # noqa: E402

REF = "/root/reference/src/openpi/training/data_loader.py"


class IndexDataset:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        i = int(i)
        return {"idx": np.int64(i), "obs": {"x": np.full((3,), i, dtype=np.float32)}}


def _indices(loader):
    return [b["idx"].tolist() for b in loader]


def test_collate_transform_and_looping():
    ds = dl.TransformedDataset(IndexDataset(10), [lambda d: {**d, "twice": d["idx"] * 2}])
    assert len(ds) == 10 and ds[3]["twice"] == 6
    batches = list(dl.TorchDataLoader(ds, 4, num_batches=5))
    assert [b["idx"].tolist() for b in batches] == [[0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3]]  # drop_last, loops
    b = batches[1]
    assert isinstance(b["obs"]["x"], torch.Tensor) and b["obs"]["x"].shape == (4, 3) and b["obs"]["x"].dtype == torch.float32
    assert b["twice"].tolist() == [8, 10, 12, 14]
    a = _indices(dl.TorchDataLoader(IndexDataset(32), 8, shuffle=True, seed=3, num_batches=6))
    assert a == _indices(dl.TorchDataLoader(IndexDataset(32), 8, shuffle=True, seed=3, num_batches=6))
    assert a != _indices(dl.TorchDataLoader(IndexDataset(32), 8, shuffle=True, seed=4, num_batches=6))
    assert sorted(sum(a[:4], [])) == list(range(32)) and a[4:] != a[:2]  # one epoch is a permutation; the next is another one
    with pytest.raises(ValueError, match="larger than the dataset size"):
        dl.TorchDataLoader(IndexDataset(3), 4)
    it = iter(dl.TorchDataLoader(IndexDataset(4), 2))  # num_batches=None: endless
    assert [next(it)["idx"].tolist() for _ in range(5)] == [[0, 1], [2, 3], [0, 1], [2, 3], [0, 1]]


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_loader_reference.npz")
REF_CASES = [(False, 0, 7), (True, 3, 9), (True, 11, 4)]


def _reference_batches(shuffle, seed, nb):
    """The reference loader's batches over IndexDataset(30), batch 4, as (idx, obs.x) arrays of shape (nb, 4) / (nb, 4, 3)."""

    def tree_map(fn, *ts):
        return {k: tree_map(fn, *(t[k] for t in ts)) for k in ts[0]} if isinstance(ts[0], dict) else fn(*ts)

    ns = {"torch": torch, "np": np, "os": os, "typing": typing, "multiprocessing": multiprocessing,
          "jax": types.SimpleNamespace(process_count=lambda: 1, tree=types.SimpleNamespace(map=tree_map),
                                       sharding=types.SimpleNamespace(Sharding=typing.Any))}  # fmt: skip
    for node in ast.parse(open(REF).read()).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in ("TorchDataLoader", "_collate_fn", "_worker_init_fn"):
            exec(compile(ast.Module([node], []), REF, "exec"), ns)
    rb = list(ns["TorchDataLoader"](IndexDataset(30), 4, shuffle=shuffle, num_batches=nb, seed=seed, framework="pytorch"))
    return torch.stack([r["idx"] for r in rb]).numpy(), torch.stack([r["obs"]["x"] for r in rb]).numpy()


@pytest.mark.parametrize("shuffle,seed,nb", REF_CASES)
def test_same_batches_as_the_reference_loader(shuffle, seed, nb):
    g = np.load(GOLD)
    ridx, rx = g[f"idx.{shuffle}.{seed}.{nb}"], g[f"x.{shuffle}.{seed}.{nb}"]
    ob = list(dl.TorchDataLoader(IndexDataset(30), 4, shuffle=shuffle, num_batches=nb, seed=seed))
    assert len(ridx) == len(ob) == nb
    for r, x, o in zip(ridx, rx, ob):
        assert torch.equal(torch.from_numpy(r), o["idx"]) and torch.equal(torch.from_numpy(x), o["obs"]["x"])


def test_fake_dataset_feeds_observation():
    from tiny import tiny_cfgs

    pcfg, _ = tiny_cfgs()
    ds = dl.FakeDataset(pcfg, 6)
    s = ds[2]
    assert s["image"]["base_0_rgb"].shape == (56, 56, 3) and s["image"]["base_0_rgb"].dtype == np.uint8
    assert s["tokenized_prompt"].dtype == np.int32 and 0 <= s["tokenized_prompt"].min() and s["tokenized_prompt"].max() < 2048
    assert s["state"].dtype == np.float32 and np.abs(s["state"]).max() <= 1.0 and s["actions"].shape == (10, 32)
    assert np.array_equal(ds[2]["actions"], s["actions"]) and not np.array_equal(ds[3]["actions"], s["actions"])  # keyed by index
    f = dl.FakeDataset(pcfg, 2, uint8_images=False, valid_masks=False)[0]  # the reference's dtypes: float NHWC images, masks False
    assert f["image"]["base_0_rgb"].dtype == np.float32 and not f["image_mask"]["base_0_rgb"] and not f["tokenized_prompt_mask"].any()
    loader = dl.create_torch_data_loader(ds, 2, num_batches=3, transforms=[transforms.PadStatesAndActions(32)])
    got = list(dl.DeviceFeeder(loader, "cpu", depth=2))
    assert len(got) == 3
    obs, actions = got[0]
    assert obs.images["base_0_rgb"].shape == (2, 3, 56, 56) and obs.images["base_0_rgb"].dtype == torch.float32  # uint8 HWC -> f32 CHW
    assert float(obs.images["base_0_rgb"].min()) >= -1.0 and float(obs.images["base_0_rgb"].max()) <= 1.0
    assert obs.tokenized_prompt.shape == (2, 24) and obs.image_masks["left_wrist_0_rgb"].all() and actions.shape == (2, 10, 32)
    assert torch.equal(got[2][1], torch.as_tensor(np.stack([ds[4]["actions"], ds[5]["actions"]])))  # order preserved through the feeder


def test_device_feeder_propagates_loader_errors():
    class Bad:
        def __iter__(self):
            yield transforms.flatten_dict  # not an (obs, actions) pair: the worker raises when it unpacks it

    with pytest.raises(TypeError):
        list(dl.DeviceFeeder(Bad(), "cpu"))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    loader = dl.create_torch_data_loader(IndexDataset(40), 8, shuffle=True, seed=5, num_batches=5)  # 5 steps = one epoch per rank
    idx = [b.tolist() for _, b in _pairs(loader)]
    torch.save(idx, os.path.join(out, f"r{rank}.pt"))
    dist.destroy_process_group()


def _pairs(loader):  # IndexDataset has no image keys: bypass Observation.from_dict, keep the sharding logic under test
    for batch in loader._data_loader:
        yield None, batch["idx"]


def test_distributed_sampler_shards_the_global_batch(tmp_path):
    world = 2
    mp.spawn(_rank_main, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(world))
    assert all(len(b) == 4 for b in r0 + r1)  # global batch 8 -> 4 per rank
    a, b = sum(r0, []), sum(r1, [])
    assert not set(a) & set(b) and sorted(a + b) == list(range(40))  # disjoint shards that cover the dataset in one epoch


if __name__ == "__main__":  # next to a checkout of the reference: record its loader's batches
    out = {}
    for shuffle, seed, nb in REF_CASES:
        out[f"idx.{shuffle}.{seed}.{nb}"], out[f"x.{shuffle}.{seed}.{nb}"] = _reference_batches(shuffle, seed, nb)
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, {k: v.shape for k, v in out.items()})
