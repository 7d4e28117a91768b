"""float64 numpy restatements of overlapped sliding-window inference (CPU only): the window placement, the cut of the
windows out of a raster series, and the blend of the windows' softmax into the raster.

The blend is written per WINDOW, as a scatter (`acc[:, oy:oy+ph, ox:ox+pw] += w * p`), deliberately the other formulation
than the kernel's per-pixel gather.  `blend_per_pixel` is a third, brute-force statement (a Python loop over pixels and
windows) that the scatter is checked against in tests/test_raster_windows.py, together with two planted faults.

Nothing here imports crop2seg_amd or oracle.
"""
import math

import numpy as np

U = 2.0 ** -24
FLIPS = {"": 0, "h": 1, "v": 2, "hv": 3}       # bit 1 mirrors the columns, bit 2 the rows


def window_origins(size, patch, stride, fault=None):
    """Origins along one axis: n = 1 if size <= patch else ceil((size - patch) / stride) + 1 windows at
    min(i * stride, max(size - patch, 0)).  fault "no_clamp": the last window keeps i * stride and hangs over the edge."""
    assert size >= 1 and 1 <= stride <= patch
    n = 1 if size <= patch else -(-(size - patch) // stride) + 1
    last = max(size - patch, 0)
    return [i * stride if fault == "no_clamp" else min(i * stride, last) for i in range(n)]


def hann(patch):
    """sin^2(pi (i + 1/2) / patch) in float64, rounded to f32 once (returned as f32)."""
    return np.array([math.sin(math.pi * (i + 0.5) / patch) ** 2 for i in range(patch)], dtype=np.float64).astype(np.float32)


def cut_windows(series, patch, stride, flip=0, fill=None):
    """series [T,C,H,W] -> [nwin,T,C,ph,pw] (same dtype, values copied), windows row-major; positions outside the raster take
    fill[c] (None: 0); flip & 2 mirrors the rows of every window, flip & 1 its columns."""
    series = np.asarray(series)
    T, C, H, W = series.shape
    (ph, pw), (sy, sx) = patch, stride
    fill = np.zeros(C, series.dtype) if fill is None else np.asarray(fill, dtype=series.dtype)
    out = []
    for oy in window_origins(H, ph, sy):
        for ox in window_origins(W, pw, sx):
            win = np.broadcast_to(fill[None, :, None, None], (T, C, ph, pw)).copy()
            src = series[:, :, oy:oy + ph, ox:ox + pw]
            win[:, :, :src.shape[2], :src.shape[3]] = src
            if flip & 2:
                win = win[:, :, ::-1, :]
            if flip & 1:
                win = win[:, :, :, ::-1]
            out.append(win)
    return np.ascontiguousarray(np.stack(out))


def softmax(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def blend(passes, H, W, patch, stride, wy=None, wx=None, fault=None):
    """passes: [(flip, logits [nwin,K,ph,pw])], the logits of every window of the raster in row-major order, each pass
    computed on windows mirrored by its flip.  Per window: softmax over K in float64, un-mirrored, times the separable taper
    wy[y1] * wx[x1] (None: 1), added into the raster at the window's origin (the part inside the raster).  Returns
    (proba [K,H,W] f64, top1 [H,W] int64, count [H,W] int64): count is the number of contributions to each pixel.
    fault "no_clamp": see window_origins; "no_unmirror": the logits of a mirrored pass are blended as they come."""
    (ph, pw), (sy, sx) = patch, stride
    oys = window_origins(H, ph, sy, "no_clamp" if fault == "no_clamp" else None)
    oxs = window_origins(W, pw, sx, "no_clamp" if fault == "no_clamp" else None)
    ty = np.ones(ph) if wy is None else np.asarray(wy, dtype=np.float64)
    tx = np.ones(pw) if wx is None else np.asarray(wx, dtype=np.float64)
    wgt = ty[:, None] * tx[None, :]
    K = np.asarray(passes[0][1]).shape[1]
    acc, wsum, count = np.zeros((K, H, W)), np.zeros((H, W)), np.zeros((H, W), np.int64)
    for flip, logits in passes:
        logits = np.asarray(logits, dtype=np.float64)
        assert logits.shape == (len(oys) * len(oxs), K, ph, pw)
        for iy, oy in enumerate(oys):
            for ix, ox in enumerate(oxs):
                p = softmax(logits[iy * len(oxs) + ix])
                if fault != "no_unmirror":
                    if flip & 2:
                        p = p[:, ::-1, :]
                    if flip & 1:
                        p = p[:, :, ::-1]
                h, w = min(ph, H - oy), min(pw, W - ox)
                acc[:, oy:oy + h, ox:ox + w] += wgt[None, :h, :w] * p[:, :h, :w]
                wsum[oy:oy + h, ox:ox + w] += wgt[:h, :w]
                count[oy:oy + h, ox:ox + w] += 1
    proba = acc / wsum[None]
    return proba, proba.argmax(axis=0).astype(np.int64), count


def blend_per_pixel(passes, H, W, patch, stride, wy=None, wx=None):
    """The same result pixel by pixel: for every pixel, every pass and every window, test the coverage and add."""
    (ph, pw), (sy, sx) = patch, stride
    oys, oxs = window_origins(H, ph, sy), window_origins(W, pw, sx)
    K = np.asarray(passes[0][1]).shape[1]
    proba = np.zeros((K, H, W))
    count = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            a, s = np.zeros(K), 0.0
            for flip, logits in passes:
                for iy, oy in enumerate(oys):
                    for ix, ox in enumerate(oxs):
                        y1, x1 = y - oy, x - ox
                        if not (0 <= y1 < ph and 0 <= x1 < pw):
                            continue
                        ly = ph - 1 - y1 if flip & 2 else y1
                        lx = pw - 1 - x1 if flip & 1 else x1
                        z = np.asarray(logits[iy * len(oxs) + ix][:, ly, lx], dtype=np.float64)
                        e = np.exp(z - z.max())
                        w = (1.0 if wy is None else float(wy[y1])) * (1.0 if wx is None else float(wx[x1]))
                        a += w * e / e.sum()
                        s += w
                        count[y, x] += 1
            proba[:, y, x] = a / s
    return proba, proba.argmax(axis=0).astype(np.int64), count


def bar(count):
    """|proba - ref| <= 1e-6 + (3 M + 1) 2^-24, M the largest number of contributions to one pixel: 1e-6 is the project's bar
    for this softmax arithmetic (tests/test_tail_gpu.py), the second term one rounding per multiply, per add into acc, per add
    into wsum, and the divide (all values are <= 1)."""
    return 1e-6 + (3 * int(np.max(count)) + 1) * U


def random_logits(gen, shape):
    """Logits as tests/test_tail_gpu.py::test_softmax_stitch_matches_restatement draws them (torch generator `gen`)."""
    import torch
    return torch.relu(2 * torch.randn(*shape, generator=gen)) * (torch.rand(*shape, generator=gen) > 0.3)
