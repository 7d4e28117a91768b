"""Fine-tuning with frozen parameters, the parts that run without a GPU: the trainable runs of TrainStep's flat buffers and
the gradient exchange over those runs (gloo, world size 2)."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from crop2seg_amd.learning.utils import clip_runs, trainable_runs  # noqa: E402


def test_trainable_runs_merge_neighbours_and_skip_frozen_slots():
    offs, total = [0, 4, 12, 16, 32], 40          # slots [0,4) [4,12) [12,16) [16,32) [32,40)
    assert trainable_runs(offs, total, [True] * 5) == [(0, 40)]
    assert trainable_runs(offs, total, [False, True, True, False, True]) == [(4, 16), (32, 40)]
    assert trainable_runs(offs, total, [True, False, True, False, False]) == [(0, 4), (12, 16)]
    assert trainable_runs(offs, total, [False] * 5) == []
    # a hole in the middle (the temporal encoder of a U-TAE frozen alone)
    assert trainable_runs(offs, total, [True, True, False, True, True]) == [(0, 12), (16, 40)]


def test_trainable_runs_split_where_the_adam_step_count_changes():
    offs, total = [0, 4, 12, 16], 20
    flags = [True, True, True, True]
    assert trainable_runs(offs, total, flags, [3, 3, 1, 1]) == [(0, 12), (12, 20)]
    assert trainable_runs(offs, total, flags, [2, 2, 2, 2]) == [(0, 20)]
    assert trainable_runs(offs, total, [True, False, True, True], [5, 5, 5, 4]) == [(0, 4), (12, 16), (16, 20)]


def test_clip_runs():
    assert clip_runs([(0, 4), (12, 16), (20, 40)], 14, 30) == [(14, 16), (20, 30)]
    assert clip_runs([(0, 4)], 4, 10) == []


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from crop2seg_amd.learning.ddp import FlatDataParallel
    offs, total = [0, 8, 24, 28, 64], 104
    flags = [True, False, True, False, True]
    g = torch.Generator().manual_seed(7 + rank)          # different gradients on every rank
    flat = torch.randn(total, generator=g)
    local = flat.clone()
    dp = FlatDataParallel()
    runs = trainable_runs(offs, total, flags)
    scale = dp.reduce_gradients(flat, runs=runs)
    full = local.clone()
    dist.all_reduce(full)
    torch.save({"flat": flat, "local": local, "full": full, "runs": runs, "scale": scale},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_exchange_over_trainable_runs_gloo_world2(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(os.path.join(tmp_path, f"rank{k}.pt")) for k in range(2)]
    assert not torch.equal(r[0]["local"], r[1]["local"])
    mask = torch.zeros(104, dtype=torch.bool)
    for b, e in r[0]["runs"]:
        mask[b:e] = True
    assert int(mask.sum()) == 8 + 4 + 40
    for k in range(2):
        assert r[k]["scale"] == 0.5
        assert torch.equal(r[k]["flat"][mask], r[k]["full"][mask]), "trainable slots differ from the full all-reduce"
        assert torch.equal(r[k]["flat"][~mask], r[k]["local"][~mask]), "a frozen slot was written"
