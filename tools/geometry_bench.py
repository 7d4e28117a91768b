"""Train step and strided-convolution kernel times for every (str_conv_k, str_conv_s, str_conv_p) geometry.

For U-TAE (B=4, T=32, 128 x 128) and TimeUNet_v1 (B=8, T=61, 128 x 128, irregular lengths as bench.py) and each geometry
(4,2,1), (2,2,0), (6,2,2):
  - the eager train step (TrainStep, median of --steps after --warmup);
  - every strided layer of the step (encoder down convolutions, decoder transposed convolutions) replayed in isolation
    with the shapes the step used: forward, and backward (data + weight gradient, one stream) timed with HIP events;
    fraction of the 157.3 TF/s fp32 MFMA peak on the FLOPs each pass executes (2 * N * Cout * Ho * Wo * Cin * k^2 per pass).
One JSON line per (model, geometry) on stdout; --out writes them to a file as well.

    python tools/geometry_bench.py [--steps 10] [--warmup 3] [--out profiles/geometry_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

PEAK = 157.3e12
GEOMETRIES = [(4, 2, 1), (2, 2, 0), (6, 2, 2)]
CASES = [("utae", 4, 32, 128), ("timeunet", 8, 61, 128)]


def _timed(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def _layer_times(E, L, rec, reps):
    """Isolated forward / backward of one recorded strided layer."""
    kind, N, cin, cout, H, W, K, pad, mode = rec
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    wshape = (cout, cin, K, K) if kind == "down" else (cin, cout, K, K)
    params = {"w": (torch.randn(wshape, generator=g) * 0.02).to(dev), "b": torch.zeros(cout, device=dev)}
    x = torch.randn(N, cin, H, W, generator=g).to(dev)
    side = E.SIDE_WGRAD
    E.SIDE_WGRAD = False

    def fwd(tape):
        ctx = E.Ctx(params, {}, {k: torch.zeros_like(v) for k, v in params.items()}, ws, True, tape)
        if kind == "down":
            return ctx, E.conv2d(ctx, [x], "w", "b", K, 2, pad, mode, None)
        return ctx, E.conv_transpose2d(ctx, x, "w", "b", K, pad)

    ws = E.Workspace(dev)
    try:
        _, out = fwd(None)
        t_fwd = _timed(lambda: fwd(None), reps)
        gout = torch.randn_like(out)

        def bwd_once():
            ctx, o = fwd(E.Tape())
            torch.cuda.synchronize()
            ctx.tape.grads[o.data_ptr()] = gout
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.tape.backward()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        bwd_once()
        t_bwd = statistics.median(bwd_once() for _ in range(reps))
    finally:
        E.SIDE_WGRAD = side
    Ho, Wo = out.shape[2], out.shape[3]
    flops = 2.0 * N * cin * cout * K * K * (Ho * Wo if kind == "down" else H * W)
    return {"layer": kind, "N": N, "cin": cin, "cout": cout, "H": H, "W": W, "k": K, "p": pad,
            "fwd_ms": round(t_fwd, 4), "bwd_ms": round(t_bwd, 4),
            "fwd_peak": round(flops / (t_fwd * 1e-3) / PEAK, 3), "bwd_peak": round(2 * flops / (t_bwd * 1e-3) / PEAK, 3)}


def run_case(model, B, T, H, geom, steps, warmup, reps):
    import crop2seg_amd as C2S
    from crop2seg_amd import _lib as L
    from crop2seg_amd import engine as E
    from crop2seg_amd.learning.synthetic import synthetic_batch
    from crop2seg_amd.learning.utils import TrainStep, default_config, get_model
    k, s, p = geom
    dev = torch.device("cuda")
    torch.manual_seed(1)
    net = get_model(default_config(model, str_conv_k=k, str_conv_s=s, str_conv_p=p)).to(dev)
    net.apply(C2S.weight_init)
    net.train()
    step = TrainStep(net, num_classes=15)
    x, dates, y, _ = synthetic_batch(B, T, H, H, 1, dev, irregular=model == "timeunet")
    # record the strided layers of one step
    recs = []
    conv2d, convt = E.conv2d, E.conv_transpose2d

    def rec_conv2d(ctx, srcs, wname, bname, K, S, pad, pad_mode, valid, need_input_grad=True):
        if S == 2:
            N_, c_, h_, w_ = srcs[0].shape
            recs.append(("down", N_, c_, ctx.p[wname].shape[0], h_, w_, K, pad, pad_mode))
        return conv2d(ctx, srcs, wname, bname, K, S, pad, pad_mode, valid, need_input_grad)

    def rec_convt(ctx, x_, wname, bname, K=4, pad=1):
        N_, c_, h_, w_ = x_.shape
        recs.append(("up", N_, c_, ctx.p[wname].shape[1], h_, w_, K, pad, L.PAD_ZEROS))
        return convt(ctx, x_, wname, bname, K, pad)

    E.conv2d, E.conv_transpose2d = rec_conv2d, rec_convt
    try:
        step(x, dates, y)
        torch.cuda.synchronize()
    finally:
        E.conv2d, E.conv_transpose2d = conv2d, convt
    for _ in range(warmup):
        step(x, dates, y)
    t_step = _timed(lambda: step(x, dates, y), steps)
    del step, net
    torch.cuda.empty_cache()
    layers = [_layer_times(E, L, r, reps) for r in dict.fromkeys(recs)]
    t_fwd = sum(r["fwd_ms"] for r in layers)
    t_bwd = sum(r["bwd_ms"] for r in layers)
    fl = sum(2.0 * r["N"] * r["cin"] * r["cout"] * r["k"] ** 2 * (r["H"] * r["W"] // 4 if r["layer"] == "down" else r["H"] * r["W"])
             for r in layers)
    return {"model": model, "B": B, "T": T, "H": H, "geometry": list(geom), "step_ms": round(t_step, 3),
            "strided_ms": round(t_fwd + t_bwd, 3), "strided_peak": round(3 * fl / ((t_fwd + t_bwd) * 1e-3) / PEAK, 3),
            "layers": layers}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for model, B, T, H in CASES:
        for geom in GEOMETRIES:
            r = run_case(model, B, T, H, geom, args.steps, args.warmup, args.reps)
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
