"""RecallCrossEntropy on the device against the default cross entropy: the loss call alone, and one U-TAE train step.

    python tools/recall_bench.py [--case loss|step] [--pairs P] [--calls N] [--steps K] [--warmup W] [--T T] [--graph] [--out FILE]

At B = 4, K = 15, 128 x 128 and at B = 8, 256 x 256:
  loss   losses.recall_ce, focal_ce (gamma 2) and smooth_ce against engine.cross_entropy, all with gradient, microseconds
         per call (device events around N back-to-back calls);
  step   TrainStep(criterion=RecallCrossEntropy(15)) against TrainStep() on two U-TAE of the same seed, ms per step, eager
         and (--graph) replayed.
Both as alternating windows in one session: P windows of each, A B A B ..., so that drift of the machine hits all alike.  Per
case one JSON line with the median of the windows and their spread (min, max): a difference inside the spread of the
default's own windows is no difference."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 128), (8, 256)]
K = 15


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def pairs(fns, n, npairs, warmup):
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(npairs):
        for f, v in zip(fns, out):
            v.append(window(f, n))
    return out


def stats(v, scale=1.0, digits=3):
    return {"median": round(statistics.median(v) * scale, digits), "min": round(min(v) * scale, digits),
            "max": round(max(v) * scale, digits)}


def loss_inputs(B, hw):
    """Seeded normal logits [B,K,hw,hw], labels in [0, K) and unit class weights, on the device (tools/loss_ab.py dumps these too)."""
    g = torch.Generator().manual_seed(B * 1000 + hw)
    z = torch.randn(B, K, hw, hw, generator=g).cuda()
    y = torch.randint(0, K, (B, hw, hw), generator=g).cuda()
    return z, y, torch.ones(K, device="cuda")


def loss_case(B, hw, a):
    from crop2seg_amd import engine as E
    from crop2seg_amd.learning import losses
    z, y, cw = loss_inputs(B, hw)
    ws = E.Workspace(z.device)
    default, recall, focal, smooth = pairs([lambda: E.cross_entropy(z, y, cw, ws, True),
                                           lambda: losses.recall_ce(z, y, 255, True, ws),
                                           lambda: losses.focal_ce(z, y, 2.0, 255, True, ws),
                                           lambda: losses.smooth_ce(z, y, 0.1, want_grad=True, ws=ws)],
                                          a.calls, a.pairs, a.warmup)
    return {"case": "loss", "B": B, "K": K, "hw": hw, "calls_per_window": a.calls, "windows": a.pairs,
            "cross_entropy_us": stats(default, 1e3, 1), "recall_ce_us": stats(recall, 1e3, 1),
            "focal_ce_us": stats(focal, 1e3, 1), "smooth_ce_us": stats(smooth, 1e3, 1)}


def build(B, T, hw, criterion):
    import crop2seg_amd as C2S
    from crop2seg_amd.learning.utils import TrainStep, weight_init
    from oracle import seeded
    torch.manual_seed(0)
    net = C2S.UTAE(input_dim=10, out_conv=[32, K])
    net.apply(weight_init)
    net = net.cuda().train()
    x, dates, y = seeded.make_inputs(B, T, 10, hw, hw, 1)
    return TrainStep(net, num_classes=K, criterion=criterion), x.cuda(), dates.cuda(), y.cuda()


def step_case(B, hw, a):
    from crop2seg_amd.learning import losses
    sd, x, dates, y = build(B, a.T, hw, None)
    sr, _, _, _ = build(B, a.T, hw, losses.RecallCrossEntropy(K, ignore_index=255))
    default, recall = pairs([lambda: sd(x, dates, y), lambda: sr(x, dates, y)], a.steps, a.pairs, a.warmup)
    rec = {"case": "step", "model": "utae", "B": B, "T": a.T, "hw": hw, "steps_per_window": a.steps, "windows": a.pairs,
           "default_eager_ms": stats(default), "recall_eager_ms": stats(recall)}
    if a.graph:
        sd.capture(x, dates, y)
        sr.capture(x, dates, y)
        default, recall = pairs([sd.replay, sr.replay], a.steps, a.pairs, a.warmup)
        rec.update(default_graph_ms=stats(default), recall_graph_ms=stats(recall))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7, help="windows of each side, alternating")
    ap.add_argument("--calls", type=int, default=200, help="loss calls per window")
    ap.add_argument("--steps", type=int, default=5, help="train steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=32, help="acquisitions per series")
    ap.add_argument("--graph", action="store_true", help="also time hipGraph replays of the step")
    ap.add_argument("--case", choices=("all", "loss", "step"), default="all", help="which of the two cases to time")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("recall_bench: needs an MI355X (no CPU fallback)")
    lines = []
    for fn in [f for name, f in (("loss", loss_case), ("step", step_case)) if a.case in ("all", name)]:
        for B, hw in SHAPES:
            rec = fn(B, hw, a)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
