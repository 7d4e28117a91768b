"""Tiled inference: the prediction loop of the reference's web app on the device.

Reference: src/webapp/prediction.py:253-355 -- a Sentinel-2 tile is cut into 10 x 10 patches of 128 x 128; the loop runs
the model on ONE patch at a time (batch_size 1), moves the logits to the host, applies Softmax(dim=1), keeps the top-1
class, stacks the 100 results, re-tiles them with einops '(h w) ... h1 w1 -> ... (h h1) (w w1)' and crops to
1098 x 1098.

Here the patches of a tile go through the backbone in batches (eval mode: BatchNorm uses running statistics, so a patch's
logits do not depend on its batch -- bit for bit, tests/test_configs_gpu.py), and one kernel (c2s_softmax_stitch) turns a
batch of logits into its part of the tile rasters: softmax, top-1, tiling and crop in a single pass, nothing leaves HBM
until the caller asks for the rasters.

predict_raster goes beyond that loop: a whole raster series of any size, uploaded once, is predicted on overlapping
windows (c2s_cut_windows), the windows' probabilities are blended with a taper and optionally averaged over mirrored
passes (c2s_softmax_blend, c2s_blend_finish) -- no seams on the patch lines, no fixed grid, nothing cut on the host.
The series may be the stored one (int16 / uint16, on the device or pinned): c2s_cut_windows_raw converts, re-orders and
normalises while it cuts, and c2s_window_frames drops, per window, the acquisitions that are empty there (swath edges).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple, Union

import torch

from . import engine as E
from ._lib import SRC_F32, SRC_I16, SRC_U16, check, lib

Tensor = torch.Tensor


@torch.no_grad()
def predict_tile(model, x: Tensor, dates: Tensor, grid: int = 10, crop: int = 1098, batch_size: int = 10,
                 parcels: Optional[Tensor] = None, boundary_homogenize: bool = False, boundary_code: int = 15,
                 parcel_mode: str = "hard", parcel_cap: Optional[int] = None):
    """x [grid*grid, T, C, h1, w1] (patches in row-major tile order, as the reference's test loader yields them), dates
    [grid*grid, T] -> (proba [K, crop, crop] f32, top1 [crop, crop] int64) on the device.
    With `parcels` ([crop, crop] parcel ids of the tile, 0 = no parcel) or `boundary_homogenize` a third element follows: the
    tile raster homogenised per parcel ([crop, crop] int64), as the web app does (crop2seg.py:335-371): by the given
    parcels (postprocess.homogenize), or by the parcels that the boundary class `boundary_code` of the stitched
    probabilities outlines (postprocess.homogenize_boundaries).  parcel_mode 'hard' votes with the top-1 pixels of every
    parcel, 'soft' with the mean of the returned probabilities over it (homogenize(type_='soft')); `parcel_cap` (the largest
    parcel id) goes to either vote as `cap`, so that a whole tile does not need a table of crop * crop rows."""
    _check_parcel_mode("predict_tile", parcel_mode, parcel_cap)
    if not x.is_cuda:
        raise RuntimeError("crop2seg_amd runs on MI355X only (no CPU fallback)")
    if parcels is not None and boundary_homogenize:
        raise ValueError("predict_tile: give `parcels` or `boundary_homogenize`, not both")
    n = x.shape[0]
    assert n == grid * grid and dates.shape[0] == n
    h1, w1 = x.shape[-2:]
    out_h, out_w = min(crop, grid * h1), min(crop, grid * w1)
    was_training = model.training
    model.eval()
    proba: Optional[Tensor] = None
    top1: Optional[Tensor] = None
    try:
        for first in range(0, n, batch_size):
            xb = x[first:first + batch_size].contiguous()
            db = dates[first:first + batch_size].contiguous()
            logits = model(xb, batch_positions=db)
            if isinstance(logits, tuple):
                logits = logits[0]
            K = logits.shape[1]
            if proba is None:
                proba = torch.empty(K, out_h, out_w, device=x.device, dtype=torch.float32)
                top1 = torch.empty(out_h, out_w, device=x.device, dtype=torch.int64)
            check(lib().c2s_softmax_stitch(logits.data_ptr(), proba.data_ptr(), top1.data_ptr(), first, logits.shape[0], K, h1, w1,
                                           grid, out_h, out_w, E._stream()), "softmax_stitch")
    finally:
        model.train(was_training)
    model.check_health()                 # one host synchronisation per tile: a failed normalisation wait must not reach a map
    return _with_homogenised(proba, top1, parcels, boundary_homogenize, boundary_code, parcel_mode, parcel_cap)


def _check_parcel_mode(who: str, parcel_mode: str, parcel_cap: Optional[int]) -> None:
    if parcel_mode not in ("hard", "soft"):
        raise ValueError(f"{who}: parcel_mode is 'hard' or 'soft', got {parcel_mode!r}")
    if parcel_cap is not None and (isinstance(parcel_cap, bool) or not isinstance(parcel_cap, int) or parcel_cap < 1):
        raise ValueError(f"{who}: parcel_cap is an int >= 1 (the largest parcel id), got {parcel_cap!r}")


def _with_homogenised(proba: Tensor, top1: Tensor, parcels: Optional[Tensor], boundary_homogenize: bool, boundary_code: int,
                      parcel_mode: str, parcel_cap: Optional[int]):
    """(proba, top1), followed by the homogenised raster where the caller asked for one."""
    if parcels is not None:
        from .postprocess import homogenize
        if parcel_mode == "soft":
            return proba, top1, homogenize(proba, parcels, proba.shape[0], cap=parcel_cap, type_="soft", from_logits=False)
        return proba, top1, homogenize(top1, parcels, proba.shape[0], cap=parcel_cap)
    if boundary_homogenize:
        from .postprocess import homogenize_boundaries
        return proba, top1, homogenize_boundaries(proba, boundary_code=boundary_code, from_logits=False)
    return proba, top1


FLIPS = {"": 0, "h": 1, "v": 2, "hv": 3}        # bit 1 mirrors x (columns), bit 2 mirrors y (rows): the kernels' `flip`


def _pair(v, name: str, who: str = "predict_raster") -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{who}: `{name}` is an int or a (y, x) pair")
        y, x = v
    else:
        y = x = v
    if isinstance(y, bool) or isinstance(x, bool) or not isinstance(y, int) or not isinstance(x, int):
        raise ValueError(f"{who}: `{name}` must be integers, got {v!r}")
    return y, x


def window_origins(size: int, patch: int, stride: int):
    """Origins of the windows along one axis, from the library's own placement (c2s_window_count / c2s_window_origin)."""
    L = lib()
    n = L.c2s_window_count(size, patch, stride)
    if n < 0:
        raise ValueError("window placement: " + L.c2s_last_error().decode(errors="replace"))
    return [L.c2s_window_origin(i, size, patch, stride) for i in range(n)]


def taper(window: str, patch: int) -> Optional[Tensor]:
    """The blend weights along one axis as f32 on the host: "hann" w[i] = sin^2(pi (i + 1/2) / patch), evaluated in float64
    and rounded once (strictly positive: a raster-border pixel under one window edge keeps a weight); "flat": None."""
    if window == "flat":
        return None
    if window != "hann":
        raise ValueError(f"predict_raster: window must be 'hann' or 'flat', got {window!r}")
    return torch.tensor([math.sin(math.pi * (i + 0.5) / patch) ** 2 for i in range(patch)], dtype=torch.float64).float()


_SRC = {torch.float32: SRC_F32, torch.int16: SRC_I16, torch.uint16: SRC_U16}       # the storage types c2s_cut_windows_raw reads


def _check_series(who: str, series) -> None:
    if not isinstance(series, Tensor) or series.dim() != 4 or series.dtype not in _SRC:
        raise ValueError(f"{who}: `series` is a [T, C, H, W] tensor of float32, int16 or uint16")


def _check_patch_stride(who: str, patch, stride) -> Tuple[int, int, int, int]:
    ph, pw = _pair(patch, "patch", who)
    sy, sx = _pair(stride, "stride", who)
    if ph < 16 or pw < 16 or ph % 8 or pw % 8:
        raise ValueError(f"{who}: patch sides must be multiples of 8, >= 16, got {(ph, pw)}")
    if not (1 <= sy <= ph and 1 <= sx <= pw):
        raise ValueError(f"{who}: need 1 <= stride <= patch, got stride {(sy, sx)} for patch {(ph, pw)}")
    return ph, pw, sy, sx


def _check_nodata(who: str, nodata, max_nodata_permille) -> None:
    if isinstance(nodata, bool) or not isinstance(nodata, (int, float)):
        raise ValueError(f"{who}: `nodata` is a number, got {nodata!r}")
    if isinstance(max_nodata_permille, bool) or not isinstance(max_nodata_permille, int) or not 0 <= max_nodata_permille <= 1000:
        raise ValueError(f"{who}: `max_nodata_permille` is an int in 0 .. 1000, got {max_nodata_permille!r}")


def _resident(who: str, series: Tensor) -> Tuple[Tensor, torch.device]:
    """The stored series where a kernel can read it: on the device, or in pinned host memory (read over PCIe, as the
    zero-copy SeriesCollator does).  After the argument checks: those need no device."""
    if series.is_cuda:
        return series.contiguous(), series.device
    try:
        pinned = series.is_pinned()
    except RuntimeError:                 # no device at all
        pinned = False
    if not pinned:
        raise RuntimeError("crop2seg_amd runs on MI355X only (no CPU fallback)")
    if not series.is_contiguous():
        raise ValueError(f"{who}: a pinned `series` must be contiguous")
    return series, torch.device("cuda", torch.cuda.current_device())


def _window_frames(L, series: Tensor, dates_dev: Tensor, dev, ph, pw, sy, sx, nwin, nodata, permille):
    T, Cs, H, W = series.shape
    nodata_px = torch.empty(nwin, T, device=dev, dtype=torch.int32)
    slots = torch.empty(nwin, T, device=dev, dtype=torch.int32)
    counts = torch.empty(nwin, device=dev, dtype=torch.int32)
    win_dates = torch.empty(nwin, T, device=dev, dtype=torch.int64)
    check(L.c2s_window_frames(series.data_ptr(), _SRC[series.dtype], dates_dev.data_ptr(), nodata_px.data_ptr(), slots.data_ptr(),
                              counts.data_ptr(), win_dates.data_ptr(), T, Cs, H, W, ph, pw, sy, sx, 0, nwin, float(nodata),
                              permille, E._stream()), "window_frames")
    return slots, counts, win_dates, nodata_px


@torch.no_grad()
def window_frames(series: Tensor, dates: Tensor, patch: Union[int, Tuple[int, int]], stride: Union[int, Tuple[int, int]],
                  nodata: float, max_nodata_permille: int = 0):
    """Which acquisitions every window of predict_raster keeps (c2s_window_frames): series [T, Cs, H, W] as stored (float32,
    int16 or uint16; on the device or pinned), dates [T] -> (slots [nwin, T] int32, counts [nwin] int32, win_dates [nwin, T]
    int64, nodata_px [nwin, T] int32) on the device, windows in row-major order.  nodata_px[w, t] counts the pixels of
    window w inside the raster where every band of frame t equals `nodata`; frame t is kept iff 1000 * nodata_px <=
    max_nodata_permille * inside; a window that would keep none keeps the frame with the fewest such pixels (lowest t on
    a tie).  slots lists the kept frames in ascending order, then -1; win_dates their dates, then 0."""
    who = "window_frames"
    _check_series(who, series)
    T, _, H, W = series.shape
    ph, pw, sy, sx = _check_patch_stride(who, patch, stride)
    _check_nodata(who, nodata, max_nodata_permille)
    if dates.numel() != T:
        raise ValueError(f"{who}: `dates` is [T]")
    series, dev = _resident(who, series)
    L = lib()
    nwin = len(window_origins(H, ph, sy)) * len(window_origins(W, pw, sx))
    dates_dev = dates.to(dev).to(torch.int64).reshape(T).contiguous()
    return _window_frames(L, series, dates_dev, dev, ph, pw, sy, sx, nwin, nodata, max_nodata_permille)


def _floats(who: str, v, n: int, name: str):
    vals = [float(a) for a in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(vals) != n:
        raise ValueError(f"{who}: `{name}` has {n} values, one per normalised channel, got {len(vals)}")
    return (ctypes.c_float * n)(*vals)


@torch.no_grad()
def predict_raster(model, series: Tensor, dates: Tensor, patch: Union[int, Tuple[int, int]] = 128,
                   stride: Union[int, Tuple[int, int]] = 96, window: str = "hann", batch_size: int = 20,
                   flips: Sequence[str] = ("",), fill: Union[float, Sequence[float]] = 0.0, parcels: Optional[Tensor] = None,
                   boundary_homogenize: bool = False, boundary_code: int = 15, parcel_mode: str = "hard",
                   parcel_cap: Optional[int] = None, channel_order: Optional[Sequence[int]] = None, mean=None, std=None,
                   ndvi: Optional[Tuple[int, int]] = None, nodata: Optional[float] = None, max_nodata_permille: int = 0,
                   pad_value: Optional[float] = None):
    """series [T, C, H, W] f32 on the device (one collated raster series, any H and W), dates [T] int64 ->
    (proba [K, H, W] f32, top1 [H, W] int64): the model run on overlapping `patch` windows every `stride` pixels (the last
    window of an axis clamped to the raster edge), the windows' softmax blended with the `window` taper and, for every entry
    of `flips` ("", "h", "v", "hv"), once more on the mirrored windows -- test-time mirroring, un-mirrored and averaged in
    with the same weights.  c2s_cut_windows cuts the windows out of the series, c2s_softmax_blend gathers a batch of logits
    into the accumulators, c2s_blend_finish normalises and takes the top-1 class; nothing leaves HBM.  The passes run flips
    outer, window batches inner, and the blend is a gather in ascending window index, so the result does not depend on
    `batch_size`, bit for bit.  `fill` (a float or one per channel) is what a window reads beyond a raster smaller than
    itself.  `parcels` / `boundary_homogenize` / `parcel_mode` / `parcel_cap` append the homogenised raster exactly as
    in predict_tile.

    The series as STORED: `series` may also be [T, Cs, H, W] int16 or uint16 (torch.int16 / torch.uint16 tensors; uint16
    is a plain torch dtype in the torch this package runs on, so a numpy array arrives through torch.from_numpy), on the
    device or in pinned host memory (then contiguous; the kernels read it over PCIe).  With a 16-bit series, or with any of
    the following arguments, the windows are cut by c2s_cut_windows_raw: output channel c is source channel
    `channel_order[c]` (default: all, in order), converted and normalised as (v - mean[c]) / std[c] (`mean` / `std` come
    together, one value per entry of the order; neither: no normalisation), `ndvi=(a, b)` appends the NDVI of the raw source
    channels a, b as the SeriesCollator does -- the arithmetic is the collate kernel's, and no fp32 copy of the raster is
    ever made.  `fill` then has one value per OUTPUT channel.  With `nodata` given, c2s_window_frames decides once, for
    every window, which acquisitions it keeps: a frame is dropped for a window when more than `max_nodata_permille` / 1000
    of the window's pixels inside the raster equal `nodata` in every band (window_frames states the rule); the kept frames
    are compacted to the front, the rest of the T frames are `pad_value` (default: the model's own spec.pad_value), which
    the model's frame flags drop, and the model gets the window's own padded dates.  Without any of this the launches are
    exactly the ones above."""
    _check_parcel_mode("predict_raster", parcel_mode, parcel_cap)
    who = "predict_raster"
    if parcels is not None and boundary_homogenize:
        raise ValueError("predict_raster: give `parcels` or `boundary_homogenize`, not both")
    _check_series(who, series)
    raw = series.dtype != torch.float32 or max_nodata_permille != 0 or any(
        v is not None for v in (channel_order, mean, std, ndvi, nodata, pad_value))
    T, Cs, H, W = series.shape
    ph, pw, sy, sx = _check_patch_stride(who, patch, stride)
    if isinstance(flips, str) or len(flips) == 0 or any(f not in FLIPS for f in flips):
        raise ValueError(f"predict_raster: flips is a non-empty sequence drawn from {sorted(FLIPS)}, got {flips!r}")
    if batch_size < 1:
        raise ValueError("predict_raster: batch_size >= 1")
    order = list(range(Cs)) if channel_order is None else [int(c) for c in channel_order]
    if any(not 0 <= c < Cs for c in order):
        raise ValueError(f"predict_raster: `channel_order` entries are source channels 0 .. {Cs - 1}, got {order}")
    if ndvi is not None and (len(ndvi) != 2 or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < Cs for c in ndvi)):
        raise ValueError(f"predict_raster: `ndvi` is a pair (a, b) of source channels 0 .. {Cs - 1}, got {ndvi!r}")
    C = len(order) + (1 if ndvi is not None else 0)
    if not order or C > 16:
        raise ValueError(f"predict_raster: 1 .. 16 channels, got {C}")
    if (mean is None) != (std is None):
        raise ValueError("predict_raster: `mean` and `std` come together")
    mean_a = None if mean is None else _floats(who, mean, len(order), "mean")
    std_a = None if std is None else _floats(who, std, len(order), "std")
    if nodata is not None or max_nodata_permille != 0:
        if nodata is None:
            raise ValueError("predict_raster: `max_nodata_permille` needs a `nodata` value")
        _check_nodata(who, nodata, max_nodata_permille)
    if pad_value is not None and (isinstance(pad_value, bool) or not isinstance(pad_value, (int, float))):
        raise ValueError(f"predict_raster: `pad_value` is a number, got {pad_value!r}")
    ty, tx = taper(window, ph), taper(window, pw)
    fills = [float(fill)] * C if isinstance(fill, (int, float)) else [float(v) for v in fill]
    if len(fills) != C:
        raise ValueError(f"predict_raster: `fill` is a float or {C} values, one per channel")
    if dates.numel() != T:
        raise ValueError("predict_raster: `dates` is [T]")
    if raw:
        series, dev = _resident(who, series)
    else:
        if not series.is_cuda:           # after the argument checks: those need no device
            raise RuntimeError("crop2seg_amd runs on MI355X only (no CPU fallback)")
        series = series.contiguous()
        dev = series.device
    L = lib()
    fill_a = (ctypes.c_float * C)(*fills)
    if ty is not None:
        ty, tx = ty.to(dev), tx.to(dev)
    ty_p, tx_p = (ty.data_ptr(), tx.data_ptr()) if ty is not None else (None, None)
    nwin = len(window_origins(H, ph, sy)) * len(window_origins(W, pw, sx))
    batch_size = min(batch_size, nwin)
    xb = torch.empty(batch_size, T, C, ph, pw, device=dev, dtype=torch.float32)
    db = dates.to(dev).reshape(1, T).repeat(batch_size, 1).contiguous()
    slots: Optional[Tensor] = None
    win_dates: Optional[Tensor] = None
    if raw:
        src_code = _SRC[series.dtype]
        order_a = (ctypes.c_int * len(order))(*order)
        na, nb = (int(ndvi[0]), int(ndvi[1])) if ndvi is not None else (-1, -1)
        if pad_value is None:
            pad_value = getattr(getattr(model, "spec", None), "pad_value", None)
        pad = 0.0 if pad_value is None else float(pad_value)
        if nodata is not None:           # once for all windows: a mirrored window keeps the same frames
            slots, _, win_dates, _ = _window_frames(L, series, db[0].to(torch.int64).contiguous(), dev, ph, pw, sy, sx, nwin,
                                                    nodata, max_nodata_permille)
    acc: Optional[Tensor] = None
    wsum: Optional[Tensor] = None
    was_training = model.training
    model.eval()
    try:
        for f in flips:
            flip = FLIPS[f]
            for first in range(0, nwin, batch_size):
                n = min(batch_size, nwin - first)
                if raw:
                    check(L.c2s_cut_windows_raw(series.data_ptr(), src_code, xb.data_ptr(),
                                                None if slots is None else slots[first:].data_ptr(), T, C, Cs, H, W, ph, pw, sy,
                                                sx, first, n, flip, order_a, mean_a, std_a, fill_a, pad, na, nb, E._stream()),
                          "cut_windows_raw")
                else:
                    check(L.c2s_cut_windows(series.data_ptr(), xb.data_ptr(), T, C, H, W, ph, pw, sy, sx, first, n, flip, fill_a,
                                            E._stream()), "cut_windows")
                logits = model(xb[:n], batch_positions=db[:n] if win_dates is None else win_dates[first:first + n])
                if isinstance(logits, tuple):
                    logits = logits[0]
                logits = logits.contiguous()
                K = logits.shape[1]
                if acc is None:
                    acc = torch.empty(K, H, W, device=dev, dtype=torch.float32)
                    wsum = torch.empty(H, W, device=dev, dtype=torch.float32)
                    check(L.c2s_fill(acc.data_ptr(), acc.numel(), 0.0, E._stream()), "fill")
                    check(L.c2s_fill(wsum.data_ptr(), wsum.numel(), 0.0, E._stream()), "fill")
                check(L.c2s_softmax_blend(logits.data_ptr(), acc.data_ptr(), wsum.data_ptr(), ty_p, tx_p, first, n, K, ph, pw, H, W,
                                          sy, sx, flip, E._stream()), "softmax_blend")
        top1 = torch.empty(H, W, device=dev, dtype=torch.int64)
        check(L.c2s_blend_finish(acc.data_ptr(), wsum.data_ptr(), top1.data_ptr(), acc.shape[0], H, W, E._stream()), "blend_finish")
    finally:
        model.train(was_training)
    model.check_health()                 # one host synchronisation per raster, as predict_tile
    proba = acc                          # the accumulator itself, finished in place
    return _with_homogenised(proba, top1, parcels, boundary_homogenize, boundary_code, parcel_mode, parcel_cap)
