"""The size-edge rows (plain data): one row per (export, limit), for test_size_rows.py (host arithmetic, no GPU) and
test_size_limits_gpu.py (the launches).

Three kinds of limit:

    L1   65,535 / 65,536 in gridDim.y or gridDim.z          quantity "planes" (N * C) or "frames" (N)
    L2   2^31 elements (2^32 bytes lie at 2^30 floats)       quantity "elements" (n) or "last_frame_base" ((N - 1) * frame)
    L3   2^32 work-items in one launch                       quantity "elements"

A row names the export, the quantity that crosses, the limit, the smallest shape that crosses it and the shape one below it,
what must happen at the crossing shape ("result": the launch computes; "refusal": C2S_EINVAL before any launch, with
`message` in c2s_last_error()), and the device bytes the crossing launch needs at its peak.  A count crosses when it is
GREATER than its limit (the limit is the last count the export takes or takes unchanged); an element count or offset
crosses when it is AT OR ABOVE its limit (the first value that needs the next bit).

Per-frame shapes come from the per-element rows of the same family (`source`), so the sub-batch of a row is already
pinned against float64 there; frame counts are the smallest N for which the quantity crosses.
"""
from typing import NamedTuple, Optional

GRID_YZ = 65535                   # the largest gridDim.y / gridDim.z the library puts in a launch
FRAMES_WINO = 65536               # frame limit of the 8-wave Winograd families (their *_supported predicates)
I32 = 1 << 31
U32 = 1 << 32


def frames_to_cross(frame: int, limit: int = I32) -> int:
    """The smallest N for which the last frame's base (N - 1) * frame is at or above `limit`."""
    return -(-limit // frame) + 1


class SizeRow(NamedTuple):
    id: str
    export: str
    quantity: str                 # "planes" | "frames" | "elements" | "last_frame_base"
    limit: int
    cross: dict                   # the smallest shape that crosses
    below: dict                   # the shape one below it
    expect: str                   # at the crossing shape: "result" | "refusal"
    message: Optional[str]        # refusal: substring of c2s_last_error()
    peak_bytes: int               # device bytes of the crossing launch (tensors of the row, sentinel frames included)
    source: str                   # the per-element row the per-frame shape comes from


def value(row: SizeRow, shape: dict) -> int:
    """The row's quantity at a shape, in Python integers."""
    if row.quantity == "planes":
        return shape["N"] * shape["C"]
    if row.quantity == "frames":
        return shape["N"]
    if row.quantity == "elements":
        return shape["n"]
    assert row.quantity == "last_frame_base", row.quantity
    return (shape["N"] - 1) * shape["frame"]


def crosses(row: SizeRow, shape: dict) -> bool:
    v = value(row, shape)
    return v > row.limit if row.quantity in ("planes", "frames") else v >= row.limit


# ------------------------------------------------------------------------------------------------ depthwise, L1
# (N, C) of a plane count: 65,537 is prime, so its planes are frames of one channel; the others keep a C that is no power of
# two where the count allows one (a swapped plane % C / plane / C shows)
DW_COUNTS = {65535: (4369, 15), 65536: (4096, 16), 65537: (65537, 1), 131070: (4369, 30), 131075: (5243, 25)}
# (K, S, pad, mode, H, W): the four builds on 8x8 planes (4 pixels per thread for the 3x3 and 4x4 kernels) and on 6x6 planes
# (1 pixel per thread); dw_ref rows k4-n130 / k6-n70 (8x8) and k3-zeros-6x6 / k4-zeros-6x6
DW_GEOMS = [(3, 1, 1, "reflect", 8, 8), (4, 2, 1, "reflect", 8, 8), (2, 2, 0, "zeros", 8, 8), (6, 2, 2, "reflect", 8, 8),
            (3, 1, 1, "zeros", 6, 6), (4, 2, 1, "zeros", 6, 6), (2, 2, 0, "zeros", 6, 6), (6, 2, 2, "reflect", 6, 6)]


def _dw_shape(planes, K, S, pad, mode, H, W):
    N, C = DW_COUNTS[planes]
    return dict(N=N, C=C, K=K, S=S, pad=pad, mode=mode, H=H, W=W)


def _dw_bytes(s):
    Ho, Wo = (s["H"] + 2 * s["pad"] - s["K"]) // s["S"] + 1, (s["W"] + 2 * s["pad"] - s["K"]) // s["S"] + 1
    planes = s["N"] * s["C"]
    # x, gout, out, two data gradients and a prior, the weight gradient's partial sums
    return 4 * (planes * (4 * s["H"] * s["W"] + 2 * Ho * Wo + s["K"] ** 2) + 2 * s["C"] * s["K"] ** 2)


def _dw_rows():
    rows = []
    for K, S, pad, mode, H, W in DW_GEOMS:
        for below, cross in ((65535, 65536), (65536, 65537), (131070, 131075)):
            sc, sb = _dw_shape(cross, K, S, pad, mode, H, W), _dw_shape(below, K, S, pad, mode, H, W)
            rows.append(SizeRow(f"dw-k{K}-{H}x{W}-{cross}", "c2s_dwconv_fwd/dgrad/wgrad", "planes", below, sc, sb, "result", None,
                                _dw_bytes(sc), "dw_ref: k4-n130, k6-n70, k3-zeros-6x6, k4-zeros-6x6"))
    return rows


# ------------------------------------------------------------------------------------------------ convolutions, L1
# 16 channels on 4x4 planes (test_conv_paths_gpu: igemm-4x4, igemm-1x1-acc; test_conv_modes_gpu: bx-4x4-acc); the Winograd
# families at the smallest planes their predicates take (wino16-ragged: 32 channels; s2-ragged: 8 channels)
def _conv_shape(N, op, chans, Cout, H, W, K, S, pad, mode, conv_mode="f32"):
    return dict(N=N, op=op, chans=chans, Cout=Cout, H=H, W=W, K=K, S=S, pad=pad, mode=mode, conv_mode=conv_mode)


def conv_out_hw(s):
    if s["op"] == "tfwd":
        return 2 * s["H"], 2 * s["W"]
    return (s["H"] + 2 * s["pad"] - s["K"]) // s["S"] + 1, (s["W"] + 2 * s["pad"] - s["K"]) // s["S"] + 1


def _conv_bytes(s):
    Ho, Wo = conv_out_hw(s)
    return 4 * (s["N"] * sum(s["chans"]) * s["H"] * s["W"] + (s["N"] + 2) * s["Cout"] * Ho * Wo + s["N"])


CONV_Z = [            # (id, family, export, shape arguments after N)
    ("igemm-1x1", "igemm", "c2s_conv_igemm", ("fwd", (16,), 16, 4, 4, 1, 1, 0, "zeros")),
    ("igemm-3x3", "igemm", "c2s_conv_igemm", ("fwd", (16,), 16, 4, 4, 3, 1, 1, "reflect")),
    ("igemm-3x3-dgrad", "igemm", "c2s_conv_igemm", ("dgrad", (16,), 16, 4, 4, 3, 1, 1, "reflect")),
    ("xpair", "xpair", "c2s_conv_xpair", ("tfwd", (16,), 16, 4, 4, 4, 2, 1, "zeros")),
    ("xpair-dgrad", "xpair", "c2s_conv_xpair", ("dgrad", (16,), 16, 8, 8, 4, 2, 1, "reflect")),
    ("bf16x3", "bf16x3", "c2s_conv3x3_bf16x3", ("fwd", (16,), 16, 4, 4, 3, 1, 1, "reflect", "bf16x3")),
    ("bf16x3-dgrad", "bf16x3", "c2s_conv3x3_bf16x3", ("dgrad", (16,), 16, 4, 4, 3, 1, 1, "reflect", "bf16x3")),
]
CONV_WINO = [
    ("wino16", "wino16", "c2s_conv3x3_winograd16", ("fwd", (32,), 64, 8, 32, 3, 1, 1, "reflect")),
    ("s2wino", "s2wino", "c2s_conv4x4s2_winograd", ("fwd", (8,), 64, 16, 64, 4, 2, 1, "reflect")),
]
Z_MESSAGE = "more than 65535 frames in one launch"
WINO_MESSAGE = "more than 65536 frames in one launch"


def _conv_rows():
    rows = []
    for rid, fam, export, args in CONV_Z:
        for cross in (65536, 65537):
            sc, sb = _conv_shape(cross, *args), _conv_shape(cross - 1, *args)
            # at 65,537 both shapes are refused: the row pins that the refusal does not wrap back into a launch
            rows.append(SizeRow(f"{rid}-{cross}", export, "frames", GRID_YZ, sc, sb, "refusal", Z_MESSAGE, 0,
                                "test_conv_paths_gpu: igemm-4x4 / xpair; test_conv_modes_gpu: bx-4x4-acc"))
    for rid, fam, export, args in CONV_WINO:
        sc, sb = _conv_shape(FRAMES_WINO + 1, *args), _conv_shape(FRAMES_WINO, *args)
        rows.append(SizeRow(f"{rid}-65537", export, "frames", FRAMES_WINO, sc, sb, "refusal", WINO_MESSAGE, _conv_bytes(sb),
                            "test_conv_paths_gpu: wino16-ragged / s2-ragged"))
    return rows


# ------------------------------------------------------------------------------------------------ convolutions, L2
# The conv kernels add 32-bit per-frame byte offsets to a 64-bit frame base: rows with the last frame's base at or above 2^31
# elements on the larger side, which also puts frames on both sides of 2^32 bytes (2^30 floats) of the input and of the output.
# Frames of 64 channels of 32 x 32 (test_conv_paths_gpu: igemm-32ch, wino16 / wino4 at their widths; test_conv_modes_gpu: bx and
# the first-layer rows at 10 channels); the stride-2 families on the planes their predicates need.  `switches`: the engine
# switches that put the shape on the family (the plan depends on them, not on N).
CONV_L2 = [           # (id, family, export, shape arguments after N, engine switches)
    ("igemm-1x1-2^31", "igemm", "c2s_conv_igemm", ("fwd", (64,), 64, 32, 32, 1, 1, 0, "zeros"), {}),
    ("igemm-3x3-2^31", "igemm", "c2s_conv_igemm", ("fwd", (64,), 64, 32, 32, 3, 1, 1, "reflect"), {"WINOGRAD": False}),
    ("igemm-3x3-dgrad-2^31", "igemm", "c2s_conv_igemm", ("dgrad", (64,), 64, 32, 32, 3, 1, 1, "reflect"), {"WINOGRAD": False}),
    ("bf16x3-2^31", "bf16x3", "c2s_conv3x3_bf16x3", ("fwd", (64,), 64, 32, 32, 3, 1, 1, "reflect", "bf16x3"), {}),
    ("bf16x3-dgrad-2^31", "bf16x3", "c2s_conv3x3_bf16x3", ("dgrad", (64,), 64, 32, 32, 3, 1, 1, "reflect", "bf16x3"), {}),
    ("wino4-2^31", "wino4", "c2s_conv3x3_winograd", ("fwd", (64,), 64, 32, 32, 3, 1, 1, "reflect"), {"WINO16": False}),
    ("wino16-2^31", "wino16", "c2s_conv3x3_winograd16", ("fwd", (64,), 64, 32, 32, 3, 1, 1, "reflect"), {}),
    ("smallcin-2^31", "smallcin", "c2s_conv3x3_smallcin", ("fwd", (10,), 64, 32, 32, 3, 1, 1, "reflect"), {}),
    ("xpair-2^31", "xpair", "c2s_conv_xpair", ("tfwd", (16,), 16, 128, 128, 4, 2, 1, "zeros"), {}),     # output 4 x the input
    ("s2wino-2^31", "s2wino", "c2s_conv4x4s2_winograd", ("fwd", (64,), 64, 64, 64, 4, 2, 1, "reflect"), {}),   # input 4 x the output
]


def conv_frames(s):
    """Elements per frame of the source and of the destination of a conv shape (the data gradient reads the output side)."""
    Ho, Wo = conv_out_hw(s)
    fi, fo = sum(s["chans"]) * s["H"] * s["W"], s["Cout"] * Ho * Wo
    return (fo, fi) if s["op"] == "dgrad" else (fi, fo)


def conv_l2_frames(s):
    """N of a CONV_L2 row -- the smallest for which the last frame's base is at or above 2^31 elements on the SMALLER side, so
    both sides cross -- and its check frames: the first, the last, and on each side the frames below and at 2^30 and 2^31
    elements (2^32 and 2^33 bytes)."""
    src, dst = conv_frames(_conv_shape(1, *s))
    N = frames_to_cross(min(src, dst))
    frames = {0, N - 1}
    for f in (src, dst):
        for lim in (1 << 30, I32):
            k = -(-lim // f)
            frames |= {k - 1, k} if k < N else set()
    return N, sorted(frames)


# the most frames each family's launcher takes (None: the frame travels in gridDim.x; any N whose tiles fit an int)
FAMILY_MAX_FRAMES = {"igemm": GRID_YZ, "xpair": GRID_YZ, "parity": GRID_YZ, "bf16x3": GRID_YZ, "wino16": FRAMES_WINO,
                     "s2wino": FRAMES_WINO, "s2dgrad": 32768, "wino4": None, "smallcin": None}

# ------------------------------------------------------------------------------------------------ other L1 refusals
OTHER_L1 = [
    SizeRow("collate-65536", "c2s_collate_series", "frames", 65535, dict(N=65536, B=1024, T=64), dict(N=65535, B=1285, T=51),
            "refusal", "too many frames for one launch", 0, "raster_raw_ref"),
    # N = n_head * B * T with n_head 16: 16 * 65 * 63 = 65,520 is the largest multiple of 16 below the limit
    SizeRow("gattn-65536", "c2s_ltae_pe_gattn", "frames", 65535, dict(N=65536, B=64, T=64), dict(N=65520, B=65, T=63),
            "refusal", "> 65535", 0, "ltae_ref"),
]

# c2s_cut_windows clamps gridDim.z at 65,535 output frames (windows x T) and loops: 16 x 16 windows at stride 1 over rasters
# whose window grid gives the count (65,537 is prime: 65,537 of the 257 x 256 windows of a single acquisition, from window 100)
def _cut_shape(frames, T, ny, nx, first=0):
    return dict(N=frames, T=T, C=2, H=15 + ny, W=15 + nx, ph=16, pw=16, first=first, nwin=frames // T)


CUT_WINDOWS = [
    SizeRow("cut-windows-65536", "c2s_cut_windows", "frames", GRID_YZ, _cut_shape(65536, 64, 32, 32), _cut_shape(65535, 51, 5, 257),
            "result", None, 4 * (65538 * 2 * 256 + 64 * 2 * 47 * 47), "test_raster_gpu"),
    SizeRow("cut-windows-65537", "c2s_cut_windows", "frames", 65536, _cut_shape(65537, 1, 257, 256, 100),
            _cut_shape(65536, 64, 32, 32), "result", None, 4 * (65539 * 2 * 256 + 2 * 272 * 271), "test_raster_gpu"),
]

# ------------------------------------------------------------------------------------------------ flat buffers, L2
_FLAT_N = I32 + 5
FLAT = [
    SizeRow("fill-2^31", "c2s_fill", "elements", I32, dict(n=_FLAT_N), dict(n=I32 - 1), "result", None, 4 * _FLAT_N, "test_ops_gpu"),
    SizeRow("add-2^31", "c2s_add_inplace", "elements", I32, dict(n=_FLAT_N), dict(n=I32 - 1), "result", None, 8 * _FLAT_N,
            "test_ops_gpu"),
    SizeRow("adam-2^31", "c2s_adam_flat", "elements", I32, dict(n=_FLAT_N), dict(n=I32 - 1), "result", None, 16 * _FLAT_N,
            "test_tail_reference_gpu"),
]


# ------------------------------------------------------------------------------------------------ frames past 2^31, L2
def _frame_row(rid, export, frame_in, frame_out, extra, source, tensors_in=1, tensors_out=1):
    """A row whose larger side crosses 2^31 elements at its last frame."""
    frame = max(frame_in, frame_out)
    N = frames_to_cross(frame)
    sc, sb = dict(N=N, frame=frame, **extra), dict(N=N - 1, frame=frame, **extra)
    peak = 4 * (tensors_in * N * frame_in + tensors_out * (N + 2) * frame_out)
    return SizeRow(rid, export, "last_frame_base", I32, sc, sb, "result", None, peak, source)


FRAMES_L2 = [
    # dw_ref k3-zeros: 6 channels of 40 x 48 (two blocks per plane of the 4-pixel kernels)
    _frame_row("dw-k3-40x48-2^31", "c2s_dwconv_fwd/dgrad", 6 * 40 * 48, 6 * 40 * 48,
               dict(C=6, K=3, S=1, pad=1, mode="zeros", H=40, W=48), "dw_ref: k3-zeros", tensors_out=2),
    # test_ops_gpu's bias add: 32 channels of 16 x 16, in place
    _frame_row("bias-add-2^31", "c2s_channel_bias_add", 0, 32 * 256, dict(C=32, HW=256), "dw_ref: k3-bias"),
    _frame_row("frame-flags-2^31", "c2s_frame_flags", 10 * 32 * 32, 0, dict(frame_elems=10 * 32 * 32), "test_ops_gpu"),
]

# ------------------------------------------------------------------------------------------------ 2^32 work-items, L3
# The launches with one thread per item and no grid-stride loop.  The aggregation has one thread per (sample, head, pixel) and
# loops over T and the channels of the group; the per-pixel GroupNorm one per (sample, group, pixel); c2s_agg_skip_term one per
# element of x.  HIP accepts a global size of 2^32 or more without an error and does not run all of it, so the exports refuse
# it; the shape below is the largest they take, and the GPU rows run that one.  (c2s_dropout_nchw caps its grid at 4096
# workgroups and strides: it has no such edge.)
_L3 = U32 + 1024
ITEMS_MESSAGE = "work-items in one launch"


def _agg_shape(B):      # norm_ref.agg_rows geometry: 16 heads, one channel per head, 32 x 32 maps from 8 x 8 attention
    return dict(n=B * 16 * 32 * 32, B=B, T=2, C=16, H=32, W=32, nh=16, h=8, w=8)


def _pgn_shape(B):      # norm_ref.pixel_gn_rows geometry: two channels per group
    return dict(n=B * 16 * 4096, B=B, C=32, HW=4096, groups=16)


def _skip_shape(B):     # TimeUNet's aggregation at 256 x 256, T = 61, 64 channels
    return dict(n=B * 61 * 64 * 256 * 256, B=B, T=61, C=64, H=256, W=256, nh=16, h=256, w=256)


_AGG_B, _PGN_B = -(-_L3 // (16 * 32 * 32)), -(-_L3 // (16 * 4096))
# (`below`: two samples fewer -- one fewer is exactly 2^32 work-items, whose last index still fits 32 bits but whose count does not)
WORK_ITEMS = [
    SizeRow("agg-fwd-2^32", "c2s_temporal_aggregate_fwd", "elements", U32, _agg_shape(_AGG_B), _agg_shape(_AGG_B - 2), "refusal",
            ITEMS_MESSAGE, 4 * _AGG_B * (2 * 16 * 1024 + 16 * 1024 + 16 * 2 * 64) + 4 * 2 * 16 * 1024, "norm_ref.agg_rows"),
    SizeRow("pixel-gn-fwd-2^32", "c2s_pixel_gn_fwd", "elements", U32, _pgn_shape(_PGN_B), _pgn_shape(_PGN_B - 2), "refusal",
            ITEMS_MESSAGE, 4 * _PGN_B * 4096 * (32 + 32 + 2 * 16) + 4 * 2 * 32 * 4096, "norm_ref.pixel_gn_rows"),
    SizeRow("agg-skip-term-2^32", "c2s_agg_skip_term", "elements", U32, _skip_shape(17), _skip_shape(16), "refusal",
            ITEMS_MESSAGE, 0, "test_s2dgrad_skip_gpu"),
]

def _conv_l2_rows():
    rows = []
    for rid, fam, export, args, sw in CONV_L2:
        N, _ = conv_l2_frames(args)
        sc, sb = _conv_shape(N, *args), _conv_shape(N - 1, *args)
        src, dst = conv_frames(sc)
        sc["frame"] = sb["frame"] = min(src, dst)
        rows.append(SizeRow(rid, export, "last_frame_base", I32, sc, sb, "result", None, 4 * (N * src + (N + 2) * dst + N),
                            "test_conv_paths_gpu / test_conv_modes_gpu rows of the family"))
    return rows


ROWS = _dw_rows() + _conv_rows() + _conv_l2_rows() + OTHER_L1 + CUT_WINDOWS + FLAT + FRAMES_L2 + WORK_ITEMS
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# ------------------------------------------------------------------------------------------------ size queries
# The packed-weight queries, from the layouts stated at their declarations in include/c2s_hip.h (Python integers):
#   c2s_winograd_packed_floats    [cout block of 64][chunk of 8 input channels][16][8][64]
#   c2s_winograd16_packed_floats  [cout block of 64][chunk of 8 input channels][8 c][4 xi][64 o][4 nu]
#   c2s_s2wino_packed_floats      [cout block][chunk of 2 channels][2][4 parities][64][12]
#   c2s_bf16x3_packed_elems       [cin / 8][10 taps][coutP][8]
PACKED_FORMULAS = {
    "c2s_winograd_packed_floats": lambda cin, coutP: (coutP // 64) * -(-cin // 8) * 16 * 8 * 64,
    "c2s_winograd16_packed_floats": lambda cin, coutP: (coutP // 64) * -(-cin // 8) * 8 * 4 * 64 * 4,
    "c2s_s2wino_packed_floats": lambda cin, coutP: (coutP // 64) * -(-cin // 2) * 2 * 4 * 64 * 12,
    "c2s_bf16x3_packed_elems": lambda cin, coutP: -(-cin // 8) * 10 * coutP * 8,
}
PACKED_SHAPES = [(8, 64), (32, 64), (64, 128), (72, 64), (128, 1024), (1024, 1024), (8192, 8192), (32768, 16384)]


# The workspace and size queries in closed form, as include/c2s_hip.h states them at its end (Python integers).
def segs(HW):
    return -(-HW // min(HW, 2048))


MAX_CLASSES = 32
WORKSPACE_FORMULAS = {
    "norm": lambda N, C, HW: 3 * N * C * segs(HW) + 6 * N * C + 64,
    "norm_onepass_sync": lambda N, C, HW: 64 + 16 * N * C * segs(HW),            # where the one-pass form takes the shape
    "se": lambda N, C, HW: N * C * segs(HW) + 2 * N * (C // 16) * C + N * C,
    "wgrad": lambda nslices, K, cin, cout: nslices * K * K * (-(-cin // 32) * 32) * (-(-cout // 64) * 64),
    "agg_bwd": lambda nh, B, T, H, W: nh * B * T * H * W,
    "pixel_gn_bwd": lambda B, C, HW: 2 * B * -(-HW // 256) * C + 2 * C,
    "cross_entropy": lambda B, HW: 3 * 512 + 3,
    "recall_ce": lambda B, HW: B * HW + 512 + (2 * (2 * MAX_CLASSES + 1) + 1) + MAX_CLASSES + 2,
}
