"""numpy restatements of the two entries that read a raster series as STORED (CPU only): which frames every window keeps
(c2s_window_frames) and the cut + convert + re-order + normalise (+ NDVI) + compaction of the windows
(c2s_cut_windows_raw).  Plain slicing and integer counting, in the style of tests/raster_ref.py, whose window placement
this file uses.  Every quantity of `window_frames` is an integer and every float of `cut_windows_raw` is one IEEE fp32
subtraction and division (numpy float32 arithmetic), so the kernels are compared bit for bit.

`window_frames` takes planted faults (tests/test_raster_raw_reference.py checks that its own cases see each of them).

Nothing here imports crop2seg_amd or oracle.
"""
import numpy as np

import raster_ref as RR

FAULTS = ("lt", "outside_inside", "any_channel", "tie_high", "unordered")


def values(rng, dtype, shape):
    """Stored values without a single 0 (the scenes' nodata): int16 with negative values, uint16 with values above 32767,
    float32 with fractions."""
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        v = rng.integers(-3000, 12000, size=shape).astype(np.int16)
    elif dtype == np.uint16:
        v = rng.integers(1, 65536, size=shape).astype(np.uint16)
    else:
        v = rng.normal(0, 1500, size=shape).astype(np.float32)
    v[v == 0] = 7
    return v


def scene(dtype, T, Cs, H, W, seed=0):
    """A series with nodata = 0 planted (T >= 3): frame 1 empty everywhere; in frame 0 an empty rectangle [0, 20) x [0, 30)
    that covers the first window wholly and its neighbours partly; in frame 2 pixels where only SOME channels are 0 (channel
    0 alone in one block, two later channels in another: never all); and in EVERY frame t a few wholly empty pixels,
    3 + t % 5 of them, in the raster's bottom-right corner, so that the last window has no complete frame and, with
    T > 5, several frames tie for the fewest empty pixels."""
    assert T >= 3 and Cs >= 4
    rng = np.random.default_rng(seed)
    s = values(rng, dtype, (T, Cs, H, W))
    s[1] = 0
    s[0, :, :20, :30] = 0
    s[2, 0, 2:9, 3:17] = 0
    s[2, 1:3, 5:H, W // 2:W // 2 + 6] = 0
    for t in range(T):
        for i in range(3 + t % 5):
            s[t, :, H - 1 - i // 4, W - 1 - i % 4] = 0
    return s


def threshold_scene(dtype, T=3, Cs=3, seed=1):
    """32 x 48, exact fit of 2 x 3 windows of 16 at stride 16 (inside = 256).  Window 2 (origin (0, 32)): frame 0 has 64 empty
    pixels, frame 1 has 65, the others none: at 250 permille frame 0 is kept (64000 <= 64000) and frame 1 dropped."""
    s = values(np.random.default_rng(seed), dtype, (T, Cs, 32, 48))
    s[0, :, 0:8, 32:40] = 0
    s[1, :, 0:8, 32:40] = 0
    s[1, :, 8, 32] = 0
    return s


def window_frames(series, dates, patch, stride, nodata, permille, fault=None):
    """series [T,Cs,H,W] (float32 / int16 / uint16), dates [T] -> (slots [nwin,T] int32, counts [nwin] int32, win_dates
    [nwin,T] int64, nodata_px [nwin,T] int32), windows row-major.  A pixel is empty when EVERY channel equals nodata;
    nodata_px counts the empty pixels of the window's part inside the raster (`inside` pixels); frame t is kept iff
    1000 * nodata_px <= permille * inside; a window that would keep none keeps the t with the smallest nodata_px, lowest t
    on a tie; slots = the kept t ascending then -1, win_dates = their dates then 0.
    Faults: "lt" (< at the threshold), "outside_inside" (inside = ph * pw whatever the raster), "any_channel" (a pixel is
    empty when SOME channel equals nodata), "tie_high" (highest t on a tie), "unordered" (kept t descending)."""
    assert fault is None or fault in FAULTS
    series = np.asarray(series)
    dates = np.asarray(dates, dtype=np.int64)
    T, Cs, H, W = series.shape
    (ph, pw), (sy, sx) = patch, stride
    hit = series.astype(np.float32) == np.float32(nodata)               # exact for the 16-bit types
    empty = hit.any(axis=1) if fault == "any_channel" else hit.all(axis=1)
    slots, counts, win_dates, nodata_px = [], [], [], []
    for oy in RR.window_origins(H, ph, sy):
        for ox in RR.window_origins(W, pw, sx):
            part = empty[:, oy:oy + ph, ox:ox + pw]
            px = [int(v) for v in part.reshape(T, -1).sum(axis=1)]
            inside = ph * pw if fault == "outside_inside" else part.shape[1] * part.shape[2]
            if fault == "lt":
                kept = [t for t in range(T) if 1000 * px[t] < permille * inside]
            else:
                kept = [t for t in range(T) if 1000 * px[t] <= permille * inside]
            if not kept:
                least = min(px)
                ties = [t for t in range(T) if px[t] == least]
                kept = [ties[-1] if fault == "tie_high" else ties[0]]
            if fault == "unordered":
                kept = kept[::-1]
            slots.append(kept + [-1] * (T - len(kept)))
            counts.append(len(kept))
            win_dates.append([int(dates[t]) for t in kept] + [0] * (T - len(kept)))
            nodata_px.append(px)
    return (np.array(slots, np.int32), np.array(counts, np.int32), np.array(win_dates, np.int64), np.array(nodata_px, np.int32))


def convert(src, order=None, mean=None, std=None, ndvi=None):
    """src [..., Cs, h, w] as stored -> [..., C, h, w] float32: channel c = float32(src[order[c]]), then (v - mean[c]) / std[c]
    in fp32 when mean / std are given; with ndvi = (a, b) one more channel (a - b) / (a + b) of the RAW channels, 0 where
    a + b == 0 or where the quotient leaves [-1, 1], not normalised (s2_ts_cz_crop.py:376-391)."""
    src = np.asarray(src)
    Cs = src.shape[-3]
    order = list(range(Cs)) if order is None else list(order)
    out = src[..., order, :, :].astype(np.float32)
    if mean is not None:
        m = np.asarray(mean, np.float32).reshape(-1, 1, 1)
        s = np.asarray(std, np.float32).reshape(-1, 1, 1)
        assert m.shape[0] == len(order) and s.shape[0] == len(order)
        out = (out - m) / s
        assert out.dtype == np.float32
    if ndvi is not None:
        a, b = src[..., ndvi[0], :, :].astype(np.float32), src[..., ndvi[1], :, :].astype(np.float32)
        total = a + b
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(total == 0, np.float32(0), (a - b) / total).astype(np.float32)
        v[(v < -1) | (v > 1)] = 0
        out = np.concatenate([out, v[..., None, :, :]], axis=-3)
    return out


def cut_windows_raw(series, patch, stride, flip=0, order=None, mean=None, std=None, fill=None, pad_value=0.0, ndvi=None,
                    slots=None):
    """series [T,Cs,H,W] as stored -> x [nwin,T,C,ph,pw] float32: per window the part inside the raster converted (see
    `convert`), the rest fill[c] (output space; None: 0), mirrored as raster_ref.cut_windows; output frame j of window w is
    frame slots[w,j] (None: j), and pad_value everywhere where slots[w,j] == -1."""
    series = np.asarray(series)
    T, Cs, H, W = series.shape
    (ph, pw), (sy, sx) = patch, stride
    C = (Cs if order is None else len(order)) + (1 if ndvi is not None else 0)
    fill = np.zeros(C, np.float32) if fill is None else np.asarray(fill, dtype=np.float32)
    assert fill.shape == (C,)
    out, w = [], 0
    for oy in RR.window_origins(H, ph, sy):
        for ox in RR.window_origins(W, pw, sx):
            win = np.broadcast_to(fill[None, :, None, None], (T, C, ph, pw)).copy()
            src = convert(series[:, :, oy:oy + ph, ox:ox + pw], order, mean, std, ndvi)
            win[:, :, :src.shape[2], :src.shape[3]] = src
            if flip & 2:
                win = win[:, :, ::-1, :]
            if flip & 1:
                win = win[:, :, :, ::-1]
            if slots is not None:
                sel = np.full((T, C, ph, pw), np.float32(pad_value), np.float32)
                for j in range(T):
                    if slots[w][j] >= 0:
                        sel[j] = win[slots[w][j]]
                win = sel
            out.append(win)
            w += 1
    return np.ascontiguousarray(np.stack(out))
