"""Cost of the guarded optimiser step (TrainStep(max_grad_norm=..., skip_nonfinite=True)) at the headline shape: U-TAE train
step, B=4, T=32, 10x128x128, synthetic batch -- eager and as a replayed hipGraph pair, guarded and unguarded, in ONE process,
the variants alternating from repetition to repetition so that clock and neighbour effects hit all of them alike.

    python tools/guard_timing.py [--steps 40] [--warmup 10] [--reps 5] [--tree DIR] [--variants eager,eager_guard,...]

The variants eager_hp, graph_hp, eager_guard_hp and graph_guard_hp add the schedule path (TrainStep(lr_schedule=, param_groups=,
weight_decay=, decoupled_weight_decay=True)): --variants eager,eager_hp,graph,graph_hp,eager_guard,eager_guard_hp,graph_guard,graph_guard_hp.

--tree DIR imports crop2seg_amd from another checkout (built there), e.g. the parent commit, which knows only the variants of
its time; compare trees by alternating runs of this script.  Every window ends in a device synchronise and is timed with the
host clock; per variant the script prints one JSON line with the per-repetition ms/step, their median, minimum and spread
(max - min).  Profiling belongs in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/guard_timing.py --reps 1).
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--variants", default="eager,eager_guard,graph,graph_guard")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=128)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import crop2seg_amd as C2S
    from crop2seg_amd.learning.synthetic import synthetic_batch
    from crop2seg_amd.learning.utils import TrainStep
    if not torch.cuda.is_available():
        raise SystemExit("guard_timing: needs an MI355X; there is no CPU path to time")
    x, dates, y, _ = synthetic_batch(args.batch, args.frames, args.size, args.size, 3, "cuda")

    def make(name):
        torch.manual_seed(1)
        net = C2S.UTAE(input_dim=10, out_conv=[32, 15]).cuda()
        net.apply(C2S.weight_init)
        net.train()
        kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if "_guard" in name else {}
        if name.endswith("_hp"):
            # the schedule path: a warm-up / cosine table, two groups (the encoder at a tenth of the rate; gains and biases
            # undecayed) and decoupled decay
            from crop2seg_amd.learning import schedules as S
            nd = set(S.no_decay_names(net))
            enc = ("in_conv.", "down_blocks.")
            kw.update(lr_schedule=S.warmup_cosine(1e-3, 20, 2000), weight_decay=1e-2, decoupled_weight_decay=True,
                      param_groups=[{"params": lambda n: n.startswith(enc) and n not in nd, "lr_mult": 0.1},
                                    {"params": sorted(nd), "weight_decay": 0}])
        step = TrainStep(net, num_classes=15, **kw)
        if name.startswith("graph"):
            step(x, dates, y)
            step.capture(x, dates, y)
            return step.replay
        return lambda: step(x, dates, y)

    names = [v for v in args.variants.split(",") if v]
    runs = {n: make(n) for n in names}

    def window(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    for n in names:
        window(runs[n], args.warmup)
    times = {n: [] for n in names}
    for _ in range(args.reps):
        for n in names:
            times[n].append(window(runs[n], args.steps))
    for n in names:
        t = times[n]
        print(json.dumps({"tree": os.path.abspath(args.tree), "variant": n, "shape": [args.batch, args.frames, 10, args.size, args.size],
                          "steps": args.steps, "ms_per_step": [round(v, 4) for v in t], "median": round(statistics.median(t), 4),
                          "min": round(min(t), 4), "spread": round(max(t) - min(t), 4)}), flush=True)


if __name__ == "__main__":
    main()
