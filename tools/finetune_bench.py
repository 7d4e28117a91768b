"""ms / step of TrainStep with frozen parameters (fine-tuning), eager and under hipGraph replay (--graph).

    python tools/finetune_bench.py [--graph] [--steps K] [--warmup W] [--out FILE]

Cases: U-TAE and W-TAE at B=4, T=32, 128x128 -- all trainable, per-frame encoder frozen (in_conv, down_blocks, and W-TAE's
spatial_reduction), decoder and head only; TimeUNet_v1 at B=8, T=61, 128x128 with irregular series lengths -- all trainable,
in_conv frozen, in_conv and temporal_encoder frozen.  One JSON line per case and mode."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DECODER = ("up_blocks.", "out_conv.")
CASES = [
    ("utae", 4, 32, "all", ()),
    ("utae", 4, 32, "encoder", ("in_conv.", "down_blocks.")),
    ("utae", 4, 32, "decoder+head only", None),
    ("wtae", 4, 32, "all", ()),
    ("wtae", 4, 32, "encoder", ("in_conv.", "down_blocks.", "spatial_reduction.")),
    ("wtae", 4, 32, "decoder+head only", None),
    ("timeunet", 8, 61, "all", ()),
    ("timeunet", 8, 61, "in_conv", ("in_conv.",)),
    ("timeunet", 8, 61, "in_conv+temporal_encoder", ("in_conv.", "temporal_encoder.")),
]


def build(model, B, T, frozen):
    import crop2seg_amd as C2S
    from crop2seg_amd.learning.utils import TrainStep, weight_init
    from oracle import seeded
    torch.manual_seed(0)
    cls = {"utae": C2S.UTAE, "wtae": C2S.WTAE, "timeunet": C2S.TimeUNet_v1}[model]
    net = cls(input_dim=10, out_conv=[32, 15])
    net.apply(weight_init)
    net = net.cuda().train()
    for n, p in net.named_parameters():
        if (n.startswith(frozen) if frozen is not None else not n.startswith(DECODER)):
            p.requires_grad_(False)
    lengths = [T - (7 * b) % 35 for b in range(B)] if model == "timeunet" else None      # irregular series
    x, dates, y = seeded.make_inputs(B, T, 10, 128, 128, 1, lengths)
    return net, TrainStep(net, num_classes=15), x.cuda(), dates.cuda(), y.cuda()


def time_steps(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", action="store_true", help="also time hipGraph replays")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="model name: run its cases only")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    for model, B, T, label, frozen in CASES:
        if a.only and model != a.only:
            continue
        net, step, x, dates, y = build(model, B, T, frozen)
        ntrain = sum(p.numel() for p in net.parameters() if p.requires_grad)
        for _ in range(a.warmup):
            step(x, dates, y)
        rec = {"model": model, "B": B, "T": T, "hw": 128, "frozen": label, "trainable_params": ntrain,
               "eager_ms": round(time_steps(lambda: step(x, dates, y), a.steps), 3)}
        if a.graph:
            step.capture(x, dates, y)
            for _ in range(a.warmup):
                step.replay()
            rec["graph_ms"] = round(time_steps(step.replay, a.steps), 3)
        rec["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del net, step
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
