#!/usr/bin/env python
"""Micro-benchmark of the kernels either side of the hot path at the sizes the reference uses:
HIP-event time per call and algorithmic bytes / time against the 8 TB/s HBM peak.
Usage (GPU box): python tools/tail_bench.py [--reps 20] [--only raster_raw]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crop2seg_amd.inference import predict_tile  # noqa: E402,F401
from crop2seg_amd.learning.losses import boundary_target, focal_ce  # noqa: E402
from crop2seg_amd.learning.metrics import StepMeters  # noqa: E402
from crop2seg_amd.utils import CHANNELS_LIKE_PASTIS, SeriesCollator  # noqa: E402
from crop2seg_amd import _lib  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def line(name, ms, nbytes, note=""):
    tb = nbytes / (ms * 1e-3) / 1e12
    print(f"{name:44s} {ms * 1e3:9.1f} us  {nbytes / 1e6:9.1f} MB  {tb:5.2f} TB/s ({100 * tb / 8:4.1f} % of 8 TB/s) {note}")


def spread(fn, reps):
    """(median, min, max) of `reps` device-timed calls after one warm-up, and the peak of torch's allocator over them."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1], torch.cuda.max_memory_allocated()


def raster_raw(reps):
    """N3 on the STORED series: 1098^2, T = 60, 10 uint16 bands, 144 windows of 128 every 96 pixels, batches of 24.
    (i) what a caller had to do before c2s_cut_windows_raw: normalise the whole raster to fp32 on the device (the collate
    kernel, the raster as one series), then the fp32 predict_raster; (ii) the raw path; (iii) the raw path with nodata = 0."""
    import ctypes as C
    import crop2seg_amd as C2S
    from crop2seg_amd.inference import predict_raster, window_frames, window_origins
    L = _lib.lib()
    dev = torch.device("cuda")
    R, T, Kr, P, S, BS = 1098, 60, 20, 128, 96, 24
    rng = np.random.default_rng(1)
    mean = rng.uniform(500, 3000, 10).astype(np.float32)
    std = rng.uniform(300, 2000, 10).astype(np.float32)
    raw = torch.from_numpy(rng.integers(1, 10000, size=(T, 10, R, R), dtype=np.uint16)).to(dev)
    dates = 5 * torch.arange(T, device=dev)
    net = C2S.TimeUNet_v1(input_dim=10, out_conv=[32, Kr]).cuda()
    net.apply(C2S.weight_init)
    net.eval()
    stream = torch.cuda.current_stream().cuda_stream
    order_a = (C.c_int * 10)(*CHANNELS_LIKE_PASTIS)
    mean_a, std_a = mean.ctypes.data_as(C.POINTER(C.c_float)), std.ctypes.data_as(C.POINTER(C.c_float))
    offsets = torch.tensor([0, T], dtype=torch.int64, device=dev)
    base = torch.cuda.memory_allocated()
    copy = T * 10 * R * R * 4
    print(f"N3 raw: stored uint16 raster {raw.numel() * 2 / 1e6:.0f} MB, its fp32 copy {copy / 1e6:.0f} MB; allocated before the rows "
          f"{base / 1e6:.0f} MB (the stored raster, the model)")

    def normalise():
        x = torch.empty(T, 10, R, R, device=dev)
        _lib.check(L.c2s_collate_series(raw.data_ptr(), _lib.SRC_U16, offsets.data_ptr(), None, x.data_ptr(), None, None, 1, T, 10,
                                        10, R * R, order_a, mean_a, std_a, 0.0, stream), "collate_series")
        return x

    kw = dict(patch=P, stride=S, batch_size=BS)
    raw_kw = dict(channel_order=CHANNELS_LIKE_PASTIS, mean=mean, std=std, **kw)
    ms_n = timed(normalise, reps)
    x32 = normalise()
    part = spread(lambda: predict_raster(net, x32, dates, **kw), reps)
    del x32
    rows = [("(i) normalise to fp32 + fp32 predict_raster", spread(lambda: predict_raster(net, normalise(), dates, **kw), reps)),
            ("(ii) raw predict_raster", spread(lambda: predict_raster(net, raw, dates, **raw_kw), reps)),
            ("(iii) raw predict_raster, nodata=0", spread(lambda: predict_raster(net, raw, dates, nodata=0, **raw_kw), reps))]
    print(f"{'    normalise alone (c2s_collate_series)':48s} {ms_n:8.2f} ms")
    print(f"{'    fp32 predict_raster alone':48s} {part[0]:8.2f} ms  (min {part[1]:.2f}, max {part[2]:.2f} of {reps})")
    for name, (med, lo, hi, peak) in rows:
        print(f"{'N3 raw ' + name:48s} {med:8.2f} ms  (min {lo:.2f}, max {hi:.2f} of {reps})  peak {peak / 1e6:8.0f} MB "
              f"({(peak - base) / 1e6:6.0f} MB above the stored raster and the model)")
    print(f"    peak (i) - peak (ii) = {(rows[0][1][3] - rows[1][1][3]) / 1e6:.0f} MB; the fp32 copy is {copy / 1e6:.0f} MB")

    # the kernels alone, all 144 windows in batches of 24
    nwin = len(window_origins(R, P, S)) ** 2
    xb = torch.empty(BS, T, 10, P, P, device=dev)
    x32 = normalise()

    def cut32():
        for first in range(0, nwin, BS):
            _lib.check(L.c2s_cut_windows(x32.data_ptr(), xb.data_ptr(), T, 10, R, R, P, P, S, S, first, min(BS, nwin - first), 0,
                                         None, stream), "cut_windows")

    def cut16(slots=None):
        for first in range(0, nwin, BS):
            _lib.check(L.c2s_cut_windows_raw(raw.data_ptr(), _lib.SRC_U16, xb.data_ptr(), None if slots is None else slots[first:].data_ptr(),
                                             T, 10, 10, R, R, P, P, S, S, first, min(BS, nwin - first), 0, order_a, mean_a, std_a,
                                             None, 0.0, -1, -1, stream), "cut_windows_raw")
    out_b = nwin * xb[0].numel() * 4
    note = "(raster read once + windows written)"
    line(f"N3 c2s_cut_windows (fp32 raster), {nwin} windows", timed(cut32, reps), x32.numel() * 4 + out_b, note)
    line(f"N3 c2s_cut_windows_raw (uint16), {nwin} windows", timed(cut16, reps), raw.numel() * 2 + out_b, note)
    slots = window_frames(raw, dates, P, S, 0, 0)[0]
    line(f"N3 c2s_cut_windows_raw with slots, {nwin} windows", timed(lambda: cut16(slots), reps), raw.numel() * 2 + out_b, note)
    line("N3 c2s_window_frames, all windows", timed(lambda: window_frames(raw, dates, P, S, 0, 0), reps), R * R * T * 2,
         "(channel 0 of the raster read once; the call allocates its 4 small outputs)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["all", "raster_raw"], default="all", help="raster_raw: only the rows on the stored series")
    a = ap.parse_args()
    if a.only == "raster_raw":
        raster_raw(max(3, a.reps // 4))
        return
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    K, H = 15, 128

    # N1: B = 8 int16 series of irregular length (BASELINE.json configs[2]) -> normalised, reordered, padded fp32 batch
    lengths = [27, 51, 31, 30, 30, 40, 48, 61]
    series = [rng.integers(0, 10000, size=(t, 10, H, H), dtype=np.int16) for t in lengths]
    dates = [np.sort(rng.integers(0, 365, size=t)).astype(np.int64) for t in lengths]
    mean = rng.uniform(500, 3000, 10).astype(np.float32)
    std = rng.uniform(300, 2000, 10).astype(np.float32)
    for mode in ("staged", "zero_copy"):
        col = SeriesCollator(CHANNELS_LIKE_PASTIS, mean, std, device="cuda", mode=mode)
        ms = timed(lambda: col(series, dates), max(3, a.reps // 4))
        raw = sum(lengths) * 10 * H * H * 2
        out = 8 * 61 * 10 * H * H * 4
        line(f"N1 SeriesCollator int16 B=8 T<=61 ({mode})", ms, raw + out,
             "(whole call: host staging memcpy + " + ("H2D copy + kernel)" if mode == "staged" else "kernel reading pinned memory)"))
    # the kernel alone, raw int16 series and the (offsets | dates) table already on the device
    import ctypes as C
    L = _lib.lib()
    total = sum(lengths)
    raw_dev = torch.from_numpy(np.concatenate(series, 0)).to(dev)
    meta = torch.tensor(np.concatenate([[0], np.cumsum(lengths), np.concatenate(dates)]), dtype=torch.int64, device=dev)
    x = torch.empty(8, 61, 10, H, H, device=dev)
    dd = torch.empty(8, 61, dtype=torch.int64, device=dev)
    valid = torch.empty(8 * 61, dtype=torch.int32, device=dev)
    order_a = (C.c_int * 10)(*CHANNELS_LIKE_PASTIS)
    mean_a, std_a = mean.ctypes.data_as(C.POINTER(C.c_float)), std.ctypes.data_as(C.POINTER(C.c_float))

    def collate_kernel():
        _lib.check(L.c2s_collate_series(raw_dev.data_ptr(), _lib.SRC_I16, meta.data_ptr(), meta.data_ptr() + 8 * 9, x.data_ptr(),
                                        dd.data_ptr(), valid.data_ptr(), 8, 61, 10, 10, H * H, order_a, mean_a, std_a, 0.0,
                                        torch.cuda.current_stream().cuda_stream), "collate_series")
    ms = timed(collate_kernel, a.reps)
    line("N1 c2s_collate_series alone (int16 in HBM)", ms, total * 10 * H * H * 2 + 8 * 61 * 10 * H * H * 4)
    del raw_dev, x

    # N2: metrics tail on the logits of one step (B = 8) and of a validation batch (B = 64)
    for B in (8, 64):
        logits = torch.randn(B, K, H, H, device=dev)
        y = torch.randint(0, K, (B, H, H), device=dev)
        loss = torch.tensor(1.0, device=dev)
        meters = StepMeters(K, device="cuda")
        ms = timed(lambda: meters.update(logits, y, loss), a.reps)
        line(f"N2 StepMeters.update B={B} (argmax, top-2, 2 cms)", ms, logits.numel() * 4 + y.numel() * 8)

    # N4: boundary target and focal CE (forward + gradient) at B = 8
    y = torch.randint(0, K, (8, H, H), device=dev)
    ms = timed(lambda: boundary_target(y), a.reps)
    line("N4 boundary_target B=8", ms, y.numel() * 8 * 2)
    logits2 = torch.randn(8, 2, H, H, device=dev)
    yb = torch.randint(0, 2, (8, H, H), device=dev)
    ms = timed(lambda: focal_ce(logits2, yb, 2.0, want_grad=True), a.reps)
    line("N4 focal_ce (+gradient) B=8, 2 classes", ms, logits2.numel() * 4 * 2 + yb.numel() * 8)

    # N3: softmax + top-1 + stitch of a 10 x 10 grid of 128 x 128 patches into a 1098 x 1098 tile (one call per batch of 10)
    lg = torch.randn(10, K, H, H, device=dev)
    probs = torch.empty(K, 1098, 1098, device=dev)
    top1 = torch.empty(1098, 1098, dtype=torch.int64, device=dev)

    def stitch():
        for first in range(0, 100, 10):
            _lib.check(L.c2s_softmax_stitch(lg.data_ptr(), probs.data_ptr(), top1.data_ptr(), first, 10, K, H, H, 10, 1098, 1098,
                                            torch.cuda.current_stream().cuda_stream), "softmax_stitch")
    ms = timed(stitch, a.reps)
    line("N3 c2s_softmax_stitch, 100 patches -> 1098^2", ms, 100 * K * H * H * 4 + K * 1098 * 1098 * 4 + 1098 * 1098 * 8)
    del lg, probs, top1

    # N3, whole raster: 1098^2, T = 60, 12 x 12 overlapping windows of 128 every 96 pixels, K = 20, batches of 20 windows
    import crop2seg_amd as C2S
    from crop2seg_amd.inference import predict_raster, window_origins
    R, T, Kr, P, S, BS = 1098, 60, 20, 128, 96, 20
    oys = window_origins(R, P, S)
    nwin = len(oys) ** 2
    stream = torch.cuda.current_stream().cuda_stream
    series = torch.randn(T, 10, R, R, device=dev)
    xb = torch.empty(BS, T, 10, P, P, device=dev)

    def cut():
        for first in range(0, nwin, BS):
            _lib.check(L.c2s_cut_windows(series.data_ptr(), xb.data_ptr(), T, 10, R, R, P, P, S, S, first, min(BS, nwin - first), 0,
                                         None, stream), "cut_windows")
    ms = timed(cut, max(3, a.reps // 4))
    line(f"N3 c2s_cut_windows, {nwin} windows of 1098^2 T=60", ms, series.numel() * 4 + nwin * xb[0].numel() * 4,
         "(raster read once + windows written)")

    lg = torch.randn(BS, Kr, P, P, device=dev)
    acc = torch.empty(Kr, R, R, device=dev)
    wsum = torch.empty(R, R, device=dev)
    top1 = torch.empty(R, R, dtype=torch.int64, device=dev)
    hann = torch.sin(math.pi * (torch.arange(P, dtype=torch.float64) + 0.5) / P).pow(2).float().to(dev)
    moved = (Kr + 1) * R * R * 4 + Kr * R * R * 4 + R * R * 8           # finish: acc, wsum in; proba, top1 out
    for first in range(0, nwin, BS):
        n = min(BS, nwin - first)
        rows = min(oys[(first + n - 1) // len(oys)] + P, R) - oys[first // len(oys)]
        moved += n * Kr * P * P * 4 + 2 * rows * R * (Kr + 1) * 4      # logits in; the batch's rows of acc / wsum in and out

    def blend():
        for first in range(0, nwin, BS):
            _lib.check(L.c2s_softmax_blend(lg.data_ptr(), acc.data_ptr(), wsum.data_ptr(), hann.data_ptr(), hann.data_ptr(), first,
                                           min(BS, nwin - first), Kr, P, P, R, R, S, S, 0, stream), "softmax_blend")
        _lib.check(L.c2s_blend_finish(acc.data_ptr(), wsum.data_ptr(), top1.data_ptr(), Kr, R, R, stream), "blend_finish")
    _lib.check(L.c2s_fill(acc.data_ptr(), acc.numel(), 0.0, stream), "fill")
    _lib.check(L.c2s_fill(wsum.data_ptr(), wsum.numel(), 0.0, stream), "fill")     # the repeats keep adding: values stay finite
    ms = timed(blend, a.reps)
    line(f"N3 c2s_softmax_blend + c2s_blend_finish, {nwin} windows", ms, moved, "(rows of acc / wsum re-read per batch)")
    del lg, acc, wsum, top1, xb

    net = C2S.TimeUNet_v1(input_dim=10, out_conv=[32, Kr]).cuda()
    net.apply(C2S.weight_init)
    net.eval()
    dates1 = 5 * torch.arange(T, device=dev)
    ms_r = timed(lambda: predict_raster(net, series, dates1, patch=P, stride=S, batch_size=BS), 3)
    padded = torch.zeros(T, 10, 10 * P, 10 * P, device=dev)             # dataset_creator pads 1098 -> 1280 with zeros
    padded[:, :, :R, :R] = series
    tiles = padded.view(T, 10, 10, P, 10, P).permute(2, 4, 0, 1, 3, 5).reshape(100, T, 10, P, P).contiguous()
    del padded
    ms_t = timed(lambda: predict_tile(net, tiles, dates1[None].repeat(100, 1), batch_size=BS), 3)
    print(f"{'N3 predict_raster 1098^2 stride 96 (' + str(nwin) + ' windows)':44s} {ms_r:9.1f} ms   predict_tile (100 patches) "
          f"{ms_t:9.1f} ms   ratio {ms_r / ms_t:5.2f} (windows alone: {nwin / 100:4.2f})")
    # batches of 20 leave a last batch of 4 windows; 24 divides 144
    ms_24 = timed(lambda: predict_raster(net, series, dates1, patch=P, stride=S, batch_size=24), 3)
    print(f"{'N3 predict_raster, batch_size 24 (6 full batches)':44s} {ms_24:9.1f} ms   ratio {ms_24 / ms_t:5.2f}")
    del net, series, tiles
    raster_raw(max(3, a.reps // 4))


if __name__ == "__main__":
    main()
