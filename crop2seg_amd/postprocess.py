"""Parcel homogenisation of predictions on the device: the raster restatement of the reference's
src/helpers/postprocess.py:377-604 (`homogenize`, `homogenize_boundaries`), which iterate() calls under --get_affine
(src/learning/utils.py:341-361,383) and the web app for a whole tile (crop2seg.py:335-371).

A parcel is a set of pixels with one integer id, an area is a pixel count.  The vector side of the reference's helpers
(shapefiles, CRS, polygonisation, rasterising an LPIS layer) stays with the caller, who supplies the id raster
(DESIGN.md section 7).

`homogenize` has both label types of the reference.  'hard' (`parcel_vote`) counts arg-max pixels per parcel.  'soft'
(`parcel_soft_vote`) restates `soften` (:238-281) and the rasterisation of its `soft_label` (:491-507): the per-parcel mean of
the K class probabilities over the pixels inside the parcel, the class of the largest mean, the runner-up
(`soft_top2_label`) and the rule that a parcel becomes background only above a mean background probability of 0.7.  What
`soften` does with geometry (the spatial join of pixel centres with polygons, CRS, the merge back into the vector layer)
stays with the caller, who rasterises the parcels and gets the per-parcel table back to write as attributes.

Everything here only enqueues HIP kernels (csrc/parcels.hip) on the current stream; `check_errors`
is the one call that synchronises.  Inputs must be HIP tensors: there is no CPU fallback.  [H,W] rasters are taken as B = 1.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from ._lib import check, lib

Tensor = torch.Tensor

_ERRORS = {}        # device -> int32 [4]: iteration-cap flag | labels outside [0,cap] | classes outside [0,K) | non-finite scores


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_hip(t: Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"crop2seg_amd post-processing runs on MI355X only (no CPU fallback): {what} must be a 'cuda' tensor")


def _errors(device) -> Tensor:
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _ERRORS:
        _ERRORS[device] = torch.zeros(4, dtype=torch.int32, device=device)
    return _ERRORS[device]


def check_errors(device="cuda") -> Tuple[int, int]:
    """The one host-synchronising reader of the device error words.  Raises when a union-find loop of `label_components`
    hit its iteration cap (memory was damaged: the labels of that call are not to be trusted); returns
    (labels outside [0,cap], classes outside [0,K)) that `parcel_vote` / `parcel_soft_vote` skipped since the last call, and
    clears these three words (not the count that `nonfinite_scores` reads)."""
    err = _errors(device)
    cap_hit, skipped, bad, _ = err.tolist()
    err[:3].zero_()
    if cap_hit:
        raise RuntimeError("crop2seg_amd.postprocess: a union-find loop of label_components hit its iteration cap")
    return skipped, bad


def nonfinite_scores(device="cuda") -> int:
    """Parcel pixels that `parcel_soft_vote` left out of their parcel's mean since the last call because one of their scores
    was NaN or infinite; clears the count (and nothing else).  Synchronises, like `check_errors`."""
    err = _errors(device)
    n = int(err[3].item())
    err[3:].zero_()
    return n


def _batched(t: Tensor, dims: int) -> Tuple[Tensor, bool]:
    if t.dim() == dims - 1:
        return t.unsqueeze(0), True
    if t.dim() != dims:
        raise ValueError(f"expected a tensor of {dims - 1} or {dims} dimensions, got {t.dim()}")
    return t, False


def _seeds(scores: Tensor, boundary_code: int, second_threshold: float, from_logits: bool,
           boundary_scores: Optional[Tensor], want_t1: bool):
    _require_hip(scores, "scores")
    scores, squeezed = _batched(scores, 4)
    scores = scores.to(torch.float32).contiguous()
    B, K, H, W = scores.shape
    if boundary_scores is not None:
        _require_hip(boundary_scores, "boundary_scores")
        boundary_scores = _batched(boundary_scores, 4)[0].to(torch.float32).contiguous()
        if tuple(boundary_scores.shape) != (B, 2, H, W):
            raise ValueError(f"boundary_scores must be [{B},2,{H},{W}], got {tuple(boundary_scores.shape)}")
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=scores.device)
    t1 = torch.empty(B, H, W, dtype=torch.int64, device=scores.device) if want_t1 else None
    check(lib().c2s_parcel_seeds(scores.data_ptr(), boundary_scores.data_ptr() if boundary_scores is not None else None,
                                 mask.data_ptr(), t1.data_ptr() if want_t1 else None, B, K, H, W, 1 if from_logits else 0,
                                 int(boundary_code), float(second_threshold), _stream()), "parcel_seeds")
    return mask, t1, squeezed


def parcel_seeds(scores: Tensor, boundary_code: int = 15, second_threshold: float = 0.3, from_logits: bool = True,
                 boundary_scores: Optional[Tensor] = None) -> Tensor:
    """The `super` mask of postprocess.py:540-551: scores [B,K,H,W] (logits, or probabilities with from_logits=False) ->
    u8 [B,H,W], 1 where a pixel is neither boundary nor background:
        not (top1 == boundary_code or (top2 == boundary_code and p_top2 > second_threshold) or top1 == 0)
    With `boundary_scores` [B,2,H,W] (the separate boundary head) a pixel is boundary when its class-1 probability is >= its
    class-0 probability or > second_threshold; boundary_code is then ignored."""
    mask, _, squeezed = _seeds(scores, boundary_code, second_threshold, from_logits, boundary_scores, False)
    return mask[0] if squeezed else mask


def label_components(mask: Tensor, min_size: int = 13) -> Tuple[Tensor, Tensor]:
    """4-connected components of a mask [B,H,W] (non-zero = set), those under min_size pixels removed (postprocess.py:
    532-536,554-560) -> (labels int32 [B,H,W], count int32 [B]): survivors are numbered 1..count[b] per image in raster order
    of their first pixel (scipy.ndimage.label's numbering when min_size = 1)."""
    _require_hip(mask, "mask")
    mask, squeezed = _batched(mask, 3)
    mask = (mask != 0).to(torch.uint8).contiguous() if mask.dtype != torch.uint8 else mask.contiguous()
    B, H, W = mask.shape
    L = lib()
    need = L.c2s_label_components_workspace_bytes(B, H, W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=mask.device)
    labels = torch.empty(B, H, W, dtype=torch.int32, device=mask.device)
    count = torch.empty(B, dtype=torch.int32, device=mask.device)
    check(L.c2s_label_components(mask.data_ptr(), labels.data_ptr(), count.data_ptr(), B, H, W, int(min_size), ws.data_ptr(),
                                 need, _errors(mask.device).data_ptr(), _stream()), "label_components")
    return (labels[0], count) if squeezed else (labels, count)


def _vote(pred: Tensor, labels: Tensor, num_classes: int, bg_share, outside: str, cap: Optional[int], min_size: int = 1):
    _require_hip(pred, "pred")
    _require_hip(labels, "labels")
    if outside not in ("zero", "keep"):
        raise ValueError("outside is 'zero' or 'keep'")
    pred, squeezed = _batched(pred, 3)
    labels = _batched(labels, 3)[0]
    if pred.shape != labels.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and labels {tuple(labels.shape)} differ in shape")
    pred = pred.to(torch.int64).contiguous()
    labels = labels.to(torch.int32).contiguous()
    B, H, W = pred.shape
    if cap is None:
        cap = H * W // max(1, int(min_size)) + 1
    L = lib()
    need = L.c2s_parcel_vote_workspace_bytes(B, int(cap), int(num_classes))
    hist = torch.empty(max(need, 16) // 4, dtype=torch.int32, device=pred.device)
    out = torch.empty_like(pred)
    parcel_class = torch.empty(B, max(int(cap), 1), dtype=torch.int32, device=pred.device)
    err = _errors(pred.device)
    check(L.c2s_parcel_vote(pred.data_ptr(), labels.data_ptr(), out.data_ptr(), parcel_class.data_ptr(), B, H, W,
                            int(num_classes), int(cap), -1.0 if bg_share is None else float(bg_share),
                            1 if outside == "keep" else 0, hist.data_ptr(), need, err.data_ptr() + 4, _stream()), "parcel_vote")
    return out, parcel_class, hist, squeezed


def parcel_vote(pred: Tensor, labels: Tensor, num_classes: int, bg_share: Optional[float] = None, outside: str = "zero",
                cap: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """One class per parcel by majority pixel count (postprocess.py:449-456,580).  pred int64 [B,H,W], labels [B,H,W]
    (0 = no parcel, ids 1..cap; cap defaults to H*W + 1 rows per image -- pass the largest id to keep the table small) ->
    (out int64 [B,H,W], parcel_class int32 [B,cap]).  Class 0 wins a parcel only when bg_share is given and its share of
    the parcel is strictly above it; ties go to the lower class.  outside: what pixels without a parcel become: 'zero' (the
    reference's rasterize(fill=0)) or 'keep' (their prediction).  Pixels with a label above cap or a class outside
    [0,num_classes) are skipped and left unwritten in `out`; `check_errors` reports how many."""
    out, parcel_class, _, squeezed = _vote(pred, labels, num_classes, bg_share, outside, cap)
    return (out[0], parcel_class[0]) if squeezed else (out, parcel_class)


def _check_soft_args(scores: Tensor, labels: Tensor, bg_mean, outside: str, cap: Optional[int]):
    """The argument checks of the soft vote: they need no device."""
    if outside not in ("zero", "keep"):
        raise ValueError("outside is 'zero' or 'keep'")
    if bg_mean is None or float(bg_mean) != float(bg_mean):
        raise ValueError("bg_mean is a number (the reference's 0.7), not None or NaN")
    if cap is not None and int(cap) < 1:
        raise ValueError(f"cap {cap} < 1")
    scores, squeezed = _batched(scores, 4)
    labels = _batched(labels, 3)[0]
    B, K, H, W = scores.shape
    if tuple(labels.shape) != (B, H, W):
        raise ValueError(f"scores {tuple(scores.shape)} need labels [{B},{H},{W}], got {tuple(labels.shape)}")
    if not 2 <= K <= 32:
        raise ValueError(f"2 <= K <= 32 classes, got {K}")
    if not scores.dtype.is_floating_point:
        raise ValueError(f"scores are floating point (probabilities or logits), got {scores.dtype}")
    return scores, labels, squeezed


def parcel_soft_vote(scores: Tensor, labels: Tensor, bg_mean: float = 0.7, from_logits: bool = True, outside: str = "zero",
                     cap: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """One class per parcel by the largest mean probability (`soften`, postprocess.py:238-281).  scores f32 [B,K,H,W]
    (logits, or probabilities with from_logits=False), labels [B,H,W] (0 = no parcel, ids 1..cap; cap as in `parcel_vote`) ->
    (out int64 [B,H,W], parcel_label int32 [B,cap], parcel_top2 int32 [B,cap], parcel_mean f32 [B,cap,K],
    parcel_pixels int32 [B,cap]).  The means are sums of 2^-32 fixed-point probabilities: bit-reproducible.  Classes are
    ordered by (mean descending, class ascending); parcel_top2 is the second, parcel_label the first -- unless the first is
    class 0 and its mean is not strictly above `bg_mean`, then the second.  Ids that no pixel carries give 0 / 0 / zeros / 0.
    outside: what pixels without a parcel become: 'zero' or 'keep' (their own top-1 class).  Pixels with a label outside
    [0,cap] are skipped and left unwritten in `out` (`check_errors`); parcel pixels with a NaN or infinite score add nothing
    to their parcel (`nonfinite_scores`)."""
    scores, labels, squeezed = _check_soft_args(scores, labels, bg_mean, outside, cap)
    _require_hip(scores, "scores")
    _require_hip(labels, "labels")
    scores = scores.to(torch.float32).contiguous()
    labels = labels.to(torch.int32).contiguous()
    B, K, H, W = scores.shape
    cap = H * W + 1 if cap is None else int(cap)
    L = lib()
    need = L.c2s_parcel_soft_vote_workspace_bytes(B, cap, K)
    dev = scores.device
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    out = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    parcel_label = torch.empty(B, cap, dtype=torch.int32, device=dev)
    parcel_top2 = torch.empty(B, cap, dtype=torch.int32, device=dev)
    parcel_mean = torch.empty(B, cap, K, dtype=torch.float32, device=dev)
    parcel_pixels = torch.empty(B, cap, dtype=torch.int32, device=dev)
    check(L.c2s_parcel_soft_vote(scores.data_ptr(), labels.data_ptr(), out.data_ptr(), parcel_label.data_ptr(),
                                 parcel_top2.data_ptr(), parcel_mean.data_ptr(), parcel_pixels.data_ptr(), B, K, H, W, cap,
                                 1 if from_logits else 0, float(bg_mean), 1 if outside == "keep" else 0, ws.data_ptr(), need,
                                 _errors(dev).data_ptr() + 4, _stream()), "parcel_soft_vote")
    res = (out, parcel_label, parcel_top2, parcel_mean, parcel_pixels)
    return tuple(t[0] for t in res) if squeezed else res


def homogenize(pred: Tensor, parcels: Tensor, num_classes: int, bg_share: Optional[float] = 0.75, outside: str = "zero",
               cap: Optional[int] = None, type_: str = "hard", from_logits: bool = True, bg_mean: float = 0.7) -> Tensor:
    """postprocess.homogenize (:377-507, array_out=True) with the LPIS layer as a rasterised id map `parcels` [B,H,W]
    (0 = no parcel).  type_='hard': `pred` is the int64 class raster; every parcel takes the class that covers most of it,
    background only above `bg_share` of it.  type_='soft': `pred` is the score tensor [B,K,H,W] (logits, or probabilities with
    from_logits=False; K must equal num_classes); every parcel takes the class of its largest mean probability, background
    only above a mean of `bg_mean` (`parcel_soft_vote`, which also returns the per-parcel table)."""
    if type_ == "hard":
        return parcel_vote(pred, parcels, num_classes, bg_share, outside, cap)[0]
    if type_ != "soft":
        raise ValueError(f"type_ is 'hard' or 'soft', got {type_!r}")
    if pred.dim() not in (3, 4) or pred.shape[-3] != num_classes:
        raise ValueError(f"type_='soft' takes scores [B,{num_classes},H,W], got {tuple(pred.shape)}")
    return parcel_soft_vote(pred, parcels, bg_mean, from_logits, outside, cap)[0]


def homogenize_boundaries(scores: Tensor, boundary_code: int = 15, second_threshold: float = 0.3, from_logits: bool = True,
                          boundary_scores: Optional[Tensor] = None, min_size: int = 13) -> Tensor:
    """postprocess.homogenize_boundaries (:510-604, array_out=True): the parcels are the 4-connected components of "neither
    boundary nor background" with at least min_size pixels; each takes the non-background class that covers most of it,
    everything else becomes 0.  scores [B,K,H,W] -> int64 [B,H,W]."""
    mask, t1, squeezed = _seeds(scores, boundary_code, second_threshold, from_logits, boundary_scores, True)
    labels, _ = label_components(mask, min_size)
    out = _vote(t1, labels, scores.shape[-3], None, "zero", None, min_size)[0]
    return out[0] if squeezed else out
