"""CPU checks of predict_raster on the stored series: the numpy restatement (tests/raster_raw_ref.py) against independent
per-pixel loops and against raster_ref.cut_windows on the numpy-normalised series, five planted faults of the frame rule
each seen by this file's own cases, and the refusals of predict_raster / window_frames and of the two C entries before
any launch."""
import ctypes

import numpy as np
import pytest
import torch

import raster_raw_ref as RW
import raster_ref as RR

PATCH = (16, 16)
ORDER = [2, 0, 1]
MEAN = np.array([900.0, -40.5, 1234.25], np.float32)
STD = np.array([310.0, 77.7, 1999.0], np.float32)


def _frames_loop(series, dates, patch, stride, nodata, permille):
    """c2s_window_frames pixel by pixel: no slicing, no numpy reductions."""
    T, Cs, H, W = series.shape
    (ph, pw), (sy, sx) = patch, stride
    slots, counts, wdates, npx = [], [], [], []
    for oy in RR.window_origins(H, ph, sy):
        for ox in RR.window_origins(W, pw, sx):
            inside, px = 0, [0] * T
            for y in range(oy, oy + ph):
                for x in range(ox, ox + pw):
                    if y >= H or x >= W:
                        continue
                    inside += 1
                    for t in range(T):
                        if all(float(series[t, c, y, x]) == float(nodata) for c in range(Cs)):
                            px[t] += 1
            kept = [t for t in range(T) if 1000 * px[t] <= permille * inside]
            if not kept:
                best = 0
                for t in range(1, T):
                    if px[t] < px[best]:
                        best = t
                kept = [best]
            slots.append(kept + [-1] * (T - len(kept)))
            counts.append(len(kept))
            wdates.append([int(dates[t]) for t in kept] + [0] * (T - len(kept)))
            npx.append(px)
    return np.array(slots, np.int32), np.array(counts, np.int32), np.array(wdates, np.int64), np.array(npx, np.int32)


def _cut_loop(series, patch, stride, flip, order, mean, std, fill, pad_value, ndvi, slots):
    """c2s_cut_windows_raw element by element, in np.float32 scalar arithmetic."""
    T, Cs, H, W = series.shape
    (ph, pw), (sy, sx) = patch, stride
    C = len(order) + (1 if ndvi is not None else 0)
    oys, oxs = RR.window_origins(H, ph, sy), RR.window_origins(W, pw, sx)
    out = np.empty((len(oys) * len(oxs), T, C, ph, pw), np.float32)
    for w in range(out.shape[0]):
        oy, ox = oys[w // len(oxs)], oxs[w % len(oxs)]
        for j in range(T):
            s = j if slots is None else int(slots[w][j])
            for c in range(C):
                for y1 in range(ph):
                    for x1 in range(pw):
                        y = oy + (ph - 1 - y1 if flip & 2 else y1)
                        x = ox + (pw - 1 - x1 if flip & 1 else x1)
                        if s < 0:
                            v = np.float32(pad_value)
                        elif y >= H or x >= W:
                            v = np.float32(0.0 if fill is None else fill[c])
                        elif ndvi is not None and c == C - 1:
                            a, b = np.float32(series[s, ndvi[0], y, x]), np.float32(series[s, ndvi[1], y, x])
                            v = np.float32(0) if a + b == 0 else (a - b) / (a + b)
                            if v < -1 or v > 1:
                                v = np.float32(0)
                        else:
                            v = np.float32(series[s, order[c], y, x])
                            if mean is not None:
                                v = (v - np.float32(mean[c])) / np.float32(std[c])
                        out[w, j, c, y1, x1] = v
    return out


# (dtype, (H, W), stride): a raster smaller than the window; 2 x 2 windows, both axes clamped, odd W
TINY = [(np.int16, (10, 21), 12), (np.uint16, (19, 23), 12), (np.float32, (10, 21), 12)]


@pytest.mark.parametrize("dtype,hw,stride", TINY)
def test_reference_frames_equal_per_pixel_loop(dtype, hw, stride):
    s = RW.scene(dtype, 7, 4, *hw, seed=3)
    dates = 10 + 7 * np.arange(7)
    for permille in (0, 250, 1000):
        got = RW.window_frames(s, dates, PATCH, (stride, stride), 0, permille)
        want = _frames_loop(s, dates, PATCH, (stride, stride), 0, permille)
        for g, w, name in zip(got, want, ("slots", "counts", "win_dates", "nodata_px")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, permille)
    slots, counts, _, _ = RW.window_frames(s, dates, PATCH, (stride, stride), 0, 0)
    assert counts.min() == 1 and bool((slots[:, 0] >= 0).all()), "no window without a frame"


@pytest.mark.parametrize("dtype,hw,stride", TINY)
def test_reference_cut_equals_per_element_loop(dtype, hw, stride):
    s = RW.scene(dtype, 3, 4, *hw, seed=4)
    st = (stride, stride)
    slots = RW.window_frames(s, np.arange(3), PATCH, st, 0, 500)[0]
    fill = [-1.5, 2.0, 0.25, 9.0]
    for flip in range(4):
        for kw in (dict(order=ORDER, mean=MEAN, std=STD, fill=fill[:3], pad_value=-7.0, ndvi=None, slots=slots),
                   dict(order=ORDER, mean=None, std=None, fill=None, pad_value=0.0, ndvi=(2, 0), slots=None),
                   dict(order=ORDER, mean=MEAN, std=STD, fill=fill, pad_value=3.0, ndvi=(1, 2), slots=slots)):
            got = RW.cut_windows_raw(s, PATCH, st, flip, **kw)
            want = _cut_loop(s, PATCH, st, flip, **kw)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (flip, kw)


@pytest.mark.parametrize("dtype", [np.int16, np.uint16, np.float32])
@pytest.mark.parametrize("hw,stride", [((37, 45), 12), ((10, 21), 12)])
def test_reference_without_nodata_equals_cut_of_the_normalised_series(dtype, hw, stride):
    s = RW.values(np.random.default_rng(5), dtype, (2, 4, *hw))
    order, mean, std = [3, 0, 2], MEAN, STD
    normalised = (s[:, order].astype(np.float32) - mean.reshape(1, 3, 1, 1)) / std.reshape(1, 3, 1, 1)
    assert normalised.dtype == np.float32
    fill = np.array([0.5, -2.0, 4.0], np.float32)
    for flip in range(4):
        got = RW.cut_windows_raw(s, PATCH, (stride, stride), flip, order, mean, std, fill)
        want = RR.cut_windows(normalised, PATCH, (stride, stride), flip, fill)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    plain = RW.cut_windows_raw(s, PATCH, (stride, stride))
    assert np.array_equal(plain, RR.cut_windows(s.astype(np.float32), PATCH, (stride, stride)))


def _fault_cases():
    """(series, stride, permille) of this file, one of which must see every planted fault."""
    cases = [(RW.scene(np.int16, 7, 4, 19, 23, seed=3), 12, p) for p in (0, 250)]
    cases.append((RW.threshold_scene(np.uint16), 16, 250))
    small = RW.values(np.random.default_rng(6), np.int16, (3, 3, 10, 21))          # inside = 210, not 256
    small[0, :, :3, :20] = 0                                                        # 60 px: 60000 > 52500, but <= 64000
    cases.append((small, 12, 250))
    ties = RW.values(np.random.default_rng(7), np.int16, (4, 3, 16, 16))
    ties[:, :, 0, :2] = 0                                                           # every frame: 2 empty pixels
    cases.append((ties, 16, 0))
    return cases


@pytest.mark.parametrize("fault", RW.FAULTS)
def test_planted_faults_are_seen(fault):
    seen = 0
    for s, stride, permille in _fault_cases():
        dates = 3 * np.arange(s.shape[0]) + 1
        good = RW.window_frames(s, dates, PATCH, (stride, stride), 0, permille)
        loop = _frames_loop(s, dates, PATCH, (stride, stride), 0, permille)
        assert all(np.array_equal(g, w) for g, w in zip(good, loop))
        bad = RW.window_frames(s, dates, PATCH, (stride, stride), 0, permille, fault=fault)
        seen += not all(np.array_equal(b, w) for b, w in zip(bad, loop))
    assert seen >= 1, f"no case of this file sees the planted fault {fault}"


def test_threshold_case_is_exact():
    s = RW.threshold_scene(np.int16)
    slots, counts, _, px = RW.window_frames(s, np.arange(3), PATCH, (16, 16), 0, 250)
    assert px[2].tolist() == [64, 65, 0] and slots[2].tolist() == [0, 2, -1] and counts[2] == 2
    assert RW.window_frames(s, np.arange(3), PATCH, (16, 16), 0, 254)[0][2].tolist() == [0, 1, 2]      # 65000 <= 65024


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
class _Never(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("the model must not run")

    def check_health(self):
        raise AssertionError("no launch, no health check")


@pytest.mark.parametrize("kw", [dict(mean=[0.0] * 10), dict(std=[1.0] * 10), dict(mean=[0.0] * 9, std=[1.0] * 9),
                                dict(channel_order=[0, 1, 2], mean=[0.0] * 10, std=[1.0] * 10),
                                dict(nodata=0, max_nodata_permille=1001), dict(nodata=0, max_nodata_permille=-1),
                                dict(nodata=0, max_nodata_permille=2.5), dict(max_nodata_permille=10), dict(nodata="0"),
                                dict(ndvi=(10, 0)), dict(ndvi=(0, -1)), dict(ndvi=(1, 2, 3)), dict(channel_order=[0, 10]),
                                dict(channel_order=[]), dict(channel_order=list(range(10)) * 2),
                                dict(ndvi=(6, 2), fill=[0.0] * 10), dict(channel_order=[2, 1, 0], fill=[0.0] * 10),
                                dict(pad_value="x"), dict(dtype=torch.float64), dict(dtype=torch.int32), dict(dtype=torch.uint8)])
def test_predict_raster_raw_bad_arguments_raise_value_error(kw):
    from crop2seg_amd.inference import predict_raster
    kw = dict(kw)
    series = torch.zeros(4, 10, 40, 40, dtype=kw.pop("dtype", torch.int16))
    model = _Never().train()
    with pytest.raises(ValueError, match="predict_raster"):
        predict_raster(model, series, torch.arange(4), patch=32, stride=24, **kw)
    assert model.training


def test_raw_path_refuses_pageable_host_memory():
    from crop2seg_amd.inference import predict_raster, window_frames
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_raster(_Never(), torch.zeros(4, 10, 40, 40, dtype=torch.int16), torch.arange(4), patch=32, stride=24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        window_frames(torch.zeros(4, 10, 40, 40, dtype=torch.uint16), torch.arange(4), 32, 24, 0)
    for bad in (dict(patch=20), dict(stride=40), dict(max_nodata_permille=1001), dict(nodata=None)):
        a = dict(patch=32, stride=24, nodata=0, max_nodata_permille=0)
        a.update(bad)
        with pytest.raises(ValueError, match="window_frames"):
            window_frames(torch.zeros(4, 10, 40, 40, dtype=torch.int16), torch.arange(4), **a)
    with pytest.raises(ValueError, match="window_frames"):
        window_frames(torch.zeros(4, 10, 40, 40, dtype=torch.int16), torch.arange(5), 32, 24, 0)


def test_c_entries_refuse_bad_arguments_without_gpu():
    """Bad arguments return C2S_EINVAL (-1) with a message naming the entry point and the limit, before any launch."""
    from crop2seg_amd import _lib
    L = _lib.lib()
    p = 4096                                                   # a non-NULL, 16-byte aligned stand-in: never dereferenced

    def refused(rc, *words):
        return rc == -1 and all(w in L.c2s_last_error() for w in words)

    okf = dict(src=p, dt=_lib.SRC_U16, dates=p, px=p, slots=p, counts=p, wd=p, T=3, Cs=11, H=37, W=45, ph=16, pw=16, sy=12,
               sx=12, first=0, n=12, nodata=0.0, permille=250)

    def frames(**kw):
        a = dict(okf, **kw)
        return L.c2s_window_frames(a["src"], a["dt"], a["dates"], a["px"], a["slots"], a["counts"], a["wd"], a["T"], a["Cs"], a["H"],
                                   a["W"], a["ph"], a["pw"], a["sy"], a["sx"], a["first"], a["n"], a["nodata"], a["permille"], None)

    for name in ("src", "dates", "px", "slots", "counts", "wd"):
        assert refused(frames(**{name: None}), b"window_frames: null"), name
    assert refused(frames(src=p + 1), b"window_frames", b"aligned") and refused(frames(src=p + 2, dt=_lib.SRC_F32), b"aligned")
    assert refused(frames(dt=3), b"window_frames", b"src_dtype") and refused(frames(dt=-1), b"window_frames", b"src_dtype")
    assert refused(frames(T=0), b"window_frames") and refused(frames(Cs=0), b"window_frames") and refused(frames(W=0), b"window_frames")
    assert refused(frames(ph=20), b"window_frames", b"multiples of 8") and refused(frames(pw=8, sx=8), b"window_frames")
    assert refused(frames(sy=0), b"window_frames", b"stride") and refused(frames(sx=17), b"window_frames", b"stride")
    assert refused(frames(permille=1001), b"window_frames", b"permille") and refused(frames(permille=-1), b"window_frames", b"permille")
    assert refused(frames(first=-1), b"window_frames") and refused(frames(n=0), b"window_frames")
    assert refused(frames(first=10, n=3), b"window_frames", b"outside")             # 3 x 4 = 12 windows

    okc = dict(src=p, dt=_lib.SRC_I16, x=p, slots=None, T=3, C=10, Cs=11, H=37, W=45, ph=16, pw=16, sy=12, sx=12, first=0, n=3,
               flip=0, order=list(range(10)), mean=None, std=None, na=-1, nb=-1)

    def cut(**kw):
        a = dict(okc, **kw)
        order = None if a["order"] is None else (ctypes.c_int * 16)(*(a["order"] + [0] * (16 - len(a["order"]))))
        fa = lambda v: None if v is None else (ctypes.c_float * 16)(*([v] * 16))
        return L.c2s_cut_windows_raw(a["src"], a["dt"], a["x"], a["slots"], a["T"], a["C"], a["Cs"], a["H"], a["W"], a["ph"], a["pw"],
                                     a["sy"], a["sx"], a["first"], a["n"], a["flip"], order, fa(a["mean"]), fa(a["std"]), None,
                                     0.0, a["na"], a["nb"], None)

    assert refused(cut(src=None), b"cut_windows_raw: null") and refused(cut(x=None), b"cut_windows_raw: null")
    assert refused(cut(src=p + 1), b"cut_windows_raw", b"aligned") and refused(cut(src=p + 2, dt=_lib.SRC_F32), b"aligned")
    assert refused(cut(dt=3), b"cut_windows_raw", b"src_dtype")
    assert refused(cut(C=17, order=list(range(11)) + [0] * 5), b"cut_windows_raw", b"C <= 16")
    assert refused(cut(T=0), b"cut_windows_raw") and refused(cut(H=0), b"cut_windows_raw") and refused(cut(Cs=0), b"cut_windows_raw")
    assert refused(cut(order=[0, 1, 2, 3, 4, 5, 6, 7, 8, 11]), b"cut_windows_raw", b"channel_order")
    assert refused(cut(order=[0, 1, 2, 3, 4, 5, 6, 7, 8, -1]), b"cut_windows_raw", b"channel_order")
    assert refused(cut(order=None, C=12), b"cut_windows_raw", b"channel_order")      # the identity order runs past Cs = 11
    assert refused(cut(na=11, nb=0, C=11), b"cut_windows_raw", b"NDVI") and refused(cut(na=3, nb=-1, C=11), b"cut_windows_raw", b"NDVI")
    assert refused(cut(mean=1.0), b"cut_windows_raw", b"mean and std") and refused(cut(std=1.0), b"cut_windows_raw", b"mean and std")
    assert refused(cut(ph=20), b"cut_windows_raw", b"multiples of 8") and refused(cut(pw=12), b"cut_windows_raw")
    assert refused(cut(ph=8, sy=8), b"cut_windows_raw")
    assert refused(cut(sy=0), b"cut_windows_raw", b"stride") and refused(cut(sx=17), b"cut_windows_raw", b"stride")
    assert refused(cut(flip=4), b"cut_windows_raw", b"flip") and refused(cut(flip=-1), b"cut_windows_raw", b"flip")
    assert refused(cut(first=-1), b"cut_windows_raw") and refused(cut(n=0), b"cut_windows_raw")
    assert refused(cut(first=10, n=3), b"cut_windows_raw", b"outside")
