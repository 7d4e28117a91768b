"""Cost of TrainStep.snapshot() at the U-TAE default model (B=4, T=32, 10x128x128, synthetic batch), in one process:

  gather_us      the device time of one snapshot's launches (header + gather), between two HIP events on the step's stream
  clone_us       the same state copied tensor by tensor (`t.clone()` of the three flat buffers, every model buffer and the
                 device counters), between two HIP events: the comparison
  clone_sd_us    `{k: v.clone() for k, v in model.state_dict().items()}` plus the two moment buffers: what a loop that keeps a
                 torch-style copy on the device would launch
  host_us        host time of one snapshot() call / of the per-tensor clones (launch overhead; no synchronisation inside)
  step_ms        ms per step over a window of steps, without snapshots, with one snapshot() every `--every` steps and with the
                 gather launches alone (no copy to the host) at the same places: the stall a step sees is
                 (with - without) * every
  copy_ms        snapshot() to the end of wait(): the copy to the pinned host blob on the side stream

    python tools/checkpoint_bench.py [--steps 40] [--warmup 10] [--reps 5] [--every 10]

Every timed window ends in a device synchronise; the variants alternate from repetition to repetition.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=128)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from crop2seg_amd.learning.synthetic import synthetic_batch
    from crop2seg_amd.learning.utils import TrainStep, default_config, get_model, weight_init
    if not torch.cuda.is_available():
        raise SystemExit("checkpoint_bench: needs an MI355X; there is no CPU path to time")
    torch.manual_seed(1)
    x, dates, y, _ = synthetic_batch(args.batch, args.frames, args.size, args.size, 3, "cuda")
    net = get_model(default_config("utae")).cuda()
    net.apply(weight_init)
    net.train()
    step = TrainStep(net, num_classes=15)
    for _ in range(args.warmup):
        step(x, dates, y)
    step.snapshot().wait()                               # plans the layout, allocates the staging blobs
    plan = step._snap_plan
    state = [t for _, t in step._snapshot_regions()]

    def events(fn, n=20):
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return statistics.median(out)

    def host(fn, n=20):
        out = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            out.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
            del keep
        return statistics.median(out)

    from crop2seg_amd import engine as E
    gather = lambda: E.snapshot_gather(plan["table"], plan["n"], plan["blobs"][0])
    clones = lambda: [t.clone() for t in state]
    clone_sd = lambda: ({k: v.clone() for k, v in net.state_dict().items()}, step.exp_avg.clone(), step.exp_avg_sq.clone())
    for fn in (gather, clones, clone_sd):
        fn()
    res = {"shape": [args.batch, args.frames, 10, args.size, args.size], "regions": plan["n"], "blob_bytes": plan["blobs"][0].numel(),
           "state_dict_tensors": len(net.state_dict()),
           "gather_us": round(events(gather), 2), "clone_us": round(events(clones), 2), "clone_sd_us": round(events(clone_sd), 2),
           "host_us": {"snapshot": round(host(step.snapshot), 1), "clone": round(host(clones), 1),
                       "clone_sd": round(host(clone_sd), 1)}}
    copies = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step.snapshot().wait()
        copies.append((time.perf_counter() - t0) * 1e3)
    res["copy_ms"] = round(statistics.median(copies), 3)

    def window(every, gather_only=False):
        torch.cuda.synchronize()
        snaps = []
        t0 = time.perf_counter()
        for k in range(args.steps):
            step(x, dates, y)
            if every and k % every == every - 1:
                if gather_only:
                    gather()                             # the launches alone: no event, no copy to the host
                else:
                    snaps = snaps[-1:] + [step.snapshot()]   # a loop keeps the last two
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    plain, snap, gath = [], [], []
    for _ in range(args.reps):
        plain.append(window(0))
        snap.append(window(args.every))
        gath.append(window(args.every, gather_only=True))
    med = statistics.median
    res["step_ms"] = {"plain": [round(v, 4) for v in plain], "with_snapshot": [round(v, 4) for v in snap],
                      "with_gather_only": [round(v, 4) for v in gath], "every": args.every,
                      "median_plain": round(med(plain), 4), "median_with": round(med(snap), 4),
                      "median_gather_only": round(med(gath), 4),
                      "stall_us_per_snapshot": round((med(snap) - med(plain)) * args.every * 1e3, 1),
                      "stall_us_per_gather": round((med(gath) - med(plain)) * args.every * 1e3, 1)}
    res["gather_vs_clone"] = "slower" if res["gather_us"] > res["clone_us"] else "faster"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
