"""Temporal aggregation in isolation at the three skip levels of the flagship step (B=4, T=32, C=64, n_head=16, attention
16 x 16): forward, backward (agg_bwd_kernel) and the adjoint of the attention upsampling, HIP-event medians with the bytes
each kernel has to move and the rate that makes.  The library has one entry point for the backward, so the adjoint is the
backward with gattn minus the backward without it, both medians of the same run.  "bits" is a sum over the int32 view of
gattn: equal between two builds means equal bits of the adjoint at that level.
    python tools/agg_bench.py            (on the GPU box)"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from crop2seg_amd import _lib

L = _lib.lib()
dev = torch.device("cuda")


def timed(fn, iters):
    ms = []
    for it in range(iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= 3:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def run(B, T, Cc, nh, H, W, h, w, iters=20):
    g = torch.Generator(dev).manual_seed(7)
    x = torch.randn(B, T, Cc, H, W, device=dev, generator=g)
    attn = torch.softmax(torch.randn(nh, B, T, h, w, device=dev, generator=g), dim=2)
    gout = torch.randn(B, Cc, H, W, device=dev, generator=g)
    out, gx, gattn = torch.empty_like(gout), torch.empty_like(x), torch.zeros_like(attn)
    d = _lib.AggDesc(B, T, Cc, H, W, nh, h, w)
    ws = torch.empty(L.c2s_temporal_aggregate_bwd_workspace_floats(C.byref(d)), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        assert L.c2s_temporal_aggregate_fwd(C.byref(d), x.data_ptr(), attn.data_ptr(), None, out.data_ptr(), st) == 0

    def bwd(ga):
        assert L.c2s_temporal_aggregate_bwd(C.byref(d), x.data_ptr(), attn.data_ptr(), None, gout.data_ptr(), gx.data_ptr(), 0,
                                            ga, ws.data_ptr(), ws.numel(), st) == 0

    bwd(gattn.data_ptr())
    torch.cuda.synchronize()
    bits = int(gattn.view(torch.int32).to(torch.int64).sum())
    tf, tb, tba = timed(fwd, iters), timed(lambda: bwd(None), iters), timed(lambda: bwd(gattn.data_ptr()), iters)
    ta = tba - tb
    mb = lambda *ts: sum(t.numel() for t in ts) * 4 / 1e6                      # noqa: E731
    rows = (("fwd", tf, mb(x, out)), ("bwd", tb, mb(x, gout, gx, ws)), ("adjoint", ta, mb(ws)))
    print(f"{H:4d} x {W:<4d}" + "".join(f"  {n} {t * 1e3:7.1f} us {m:7.1f} MB ({m / t / 1e3:5.2f} TB/s)" for n, t, m in rows)
          + f"  bits {bits}", flush=True)


for hw in (128, 64, 32):
    run(4, 32, 64, 16, hw, hw, 16, 16)
