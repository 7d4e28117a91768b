"""Child process of tests/test_guard_gpu.py: the guarded step (TrainStep(max_grad_norm=..., skip_nonfinite=True)) inside a
world-size-1 "nccl" process group, next to the same guarded step without a group, from the same initial state.

The process group is created before anything else touches the GPU.  With one rank the gradient exchange (forced with
C2S_BENCH_FORCE_DIST=1 so that the RCCL kernel really runs: two overlapped buckets in the eager step, one collective between the
two graphs of a replay) is the identity and the norm is taken behind it, so decisions, parameters, moments and BatchNorm
statistics must agree bit for bit -- on clean steps (clipping active) and on a NaN batch (skipped), eager step against eager
step and replay against replay (both steps captured: a replayed step and an eager twin run side by side in one process are
not compared here).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", rank))
    dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    import crop2seg_amd as C2S
    from crop2seg_amd.learning.utils import TrainStep
    from crop2seg_amd.learning.synthetic import synthetic_batch
    from oracle import seeded

    def fresh(distributed):
        torch.manual_seed(1)
        net = C2S.UTAE(input_dim=10, out_conv=[32, 15])
        ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict(seeded.make_state(ks, 7, "tame"))
        net = net.cuda().train()
        net.spec.attn_dropout = 0.0
        net.spec.mlp_dropout = 0.0
        return net, TrainStep(net, num_classes=15, distributed=distributed, max_grad_norm=1e-2, skip_nonfinite=True)

    x, dates, y, _ = synthetic_batch(2, 6, 32, 32, 1 + rank, "cuda", lengths=[6, 4])
    xn = x.clone()
    xn[0, 1, 2, 3, 4] = float("nan")
    net_d, step_d = fresh(True)
    net_p, step_p = fresh(False)
    assert step_d.dp is not None and step_d.dp.world == world and step_d.dp.active

    def same(what):
        torch.cuda.synchronize()
        for name in ("flat_param", "exp_avg", "exp_avg_sq", "flat_buf", "slot_steps_dev", "_status"):
            a, b = getattr(step_d, name), getattr(step_p, name)
            assert bool((a.view(torch.int32) == b.view(torch.int32)).all()), f"{what}: {name} differs"
        assert step_d.skipped_steps() == step_p.skipped_steps()

    for it, xb in enumerate((x, x, xn, x)):
        ld, _ = step_d(xb, dates, y)
        lp, _ = step_p(xb, dates, y)
        same(f"eager step {it}")
    assert step_d._early_off > 0, "the early bucket was never started"
    assert step_d.skipped_steps() == 1 and float(step_d.last_clip_coef) < 1.0
    step_d.capture(x, dates, y)
    step_p.capture(x, dates, y)
    for it, xb in enumerate((x, xn, x)):
        lg, _ = step_d.replay(xb, dates, y)
        lq, _ = step_p.replay(xb, dates, y)
        same(f"replay {it}")
    assert step_d.skipped_steps() == 2
    assert float(lg) == float(lq) and bool(torch.isfinite(step_d.flat_param).all())
    dist.barrier()
    dist.destroy_process_group()
    print(f"GUARD_DIST_OK rank {rank} world {world} loss {float(lg):.6f} skipped {step_d.skipped_steps()}")


if __name__ == "__main__":
    main()
