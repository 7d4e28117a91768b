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
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple, Union

import torch

from . import engine as E
from ._lib import check, lib

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


def _pair(v, name: str) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"predict_raster: `{name}` is an int or a (y, x) pair")
        y, x = v
    else:
        y = x = v
    if isinstance(y, bool) or isinstance(x, bool) or not isinstance(y, int) or not isinstance(x, int):
        raise ValueError(f"predict_raster: `{name}` must be integers, got {v!r}")
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


@torch.no_grad()
def predict_raster(model, series: Tensor, dates: Tensor, patch: Union[int, Tuple[int, int]] = 128,
                   stride: Union[int, Tuple[int, int]] = 96, window: str = "hann", batch_size: int = 20,
                   flips: Sequence[str] = ("",), fill: Union[float, Sequence[float]] = 0.0, parcels: Optional[Tensor] = None,
                   boundary_homogenize: bool = False, boundary_code: int = 15, parcel_mode: str = "hard",
                   parcel_cap: Optional[int] = None):
    """series [T, C, H, W] f32 on the device (one collated raster series, any H and W), dates [T] int64 ->
    (proba [K, H, W] f32, top1 [H, W] int64): the model run on overlapping `patch` windows every `stride` pixels (the last
    window of an axis clamped to the raster edge), the windows' softmax blended with the `window` taper and, for every entry
    of `flips` ("", "h", "v", "hv"), once more on the mirrored windows -- test-time mirroring, un-mirrored and averaged in
    with the same weights.  c2s_cut_windows cuts the windows out of the series, c2s_softmax_blend gathers a batch of logits
    into the accumulators, c2s_blend_finish normalises and takes the top-1 class; nothing leaves HBM.  The passes run flips
    outer, window batches inner, and the blend is a gather in ascending window index, so the result does not depend on
    `batch_size`, bit for bit.  `fill` (a float or one per channel) is what a window reads beyond a raster smaller than
    itself.  `parcels` / `boundary_homogenize` / `parcel_mode` / `parcel_cap` append the homogenised raster exactly as
    in predict_tile."""
    _check_parcel_mode("predict_raster", parcel_mode, parcel_cap)
    if parcels is not None and boundary_homogenize:
        raise ValueError("predict_raster: give `parcels` or `boundary_homogenize`, not both")
    if series.dim() != 4 or series.dtype != torch.float32:
        raise ValueError("predict_raster: `series` is [T, C, H, W] float32")
    T, C, H, W = series.shape
    ph, pw = _pair(patch, "patch")
    sy, sx = _pair(stride, "stride")
    if ph < 16 or pw < 16 or ph % 8 or pw % 8:
        raise ValueError(f"predict_raster: patch sides must be multiples of 8, >= 16, got {(ph, pw)}")
    if not (1 <= sy <= ph and 1 <= sx <= pw):
        raise ValueError(f"predict_raster: need 1 <= stride <= patch, got stride {(sy, sx)} for patch {(ph, pw)}")
    if isinstance(flips, str) or len(flips) == 0 or any(f not in FLIPS for f in flips):
        raise ValueError(f"predict_raster: flips is a non-empty sequence drawn from {sorted(FLIPS)}, got {flips!r}")
    if batch_size < 1:
        raise ValueError("predict_raster: batch_size >= 1")
    if C > 16:
        raise ValueError("predict_raster: at most 16 channels")
    ty, tx = taper(window, ph), taper(window, pw)
    fills = [float(fill)] * C if isinstance(fill, (int, float)) else [float(v) for v in fill]
    if len(fills) != C:
        raise ValueError(f"predict_raster: `fill` is a float or {C} values, one per channel")
    if dates.numel() != T:
        raise ValueError("predict_raster: `dates` is [T]")
    if not series.is_cuda:               # after the argument checks: those need no device
        raise RuntimeError("crop2seg_amd runs on MI355X only (no CPU fallback)")
    L = lib()
    fill_a = (ctypes.c_float * C)(*fills)
    series = series.contiguous()
    dev = series.device
    if ty is not None:
        ty, tx = ty.to(dev), tx.to(dev)
    ty_p, tx_p = (ty.data_ptr(), tx.data_ptr()) if ty is not None else (None, None)
    nwin = len(window_origins(H, ph, sy)) * len(window_origins(W, pw, sx))
    batch_size = min(batch_size, nwin)
    xb = torch.empty(batch_size, T, C, ph, pw, device=dev, dtype=torch.float32)
    db = dates.to(dev).reshape(1, T).repeat(batch_size, 1).contiguous()
    acc: Optional[Tensor] = None
    wsum: Optional[Tensor] = None
    was_training = model.training
    model.eval()
    try:
        for f in flips:
            flip = FLIPS[f]
            for first in range(0, nwin, batch_size):
                n = min(batch_size, nwin - first)
                check(L.c2s_cut_windows(series.data_ptr(), xb.data_ptr(), T, C, H, W, ph, pw, sy, sx, first, n, flip, fill_a,
                                        E._stream()), "cut_windows")
                logits = model(xb[:n], batch_positions=db[:n])
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
