"""The rows of the depthwise-convolution tests (test_dw_plan.py without a GPU, test_dw_reference_gpu.py with one): the table,
its input generator, the pixels per thread each row's three exports must launch (c2s_dwconv_paths: the table at its
declaration in include/c2s_hip.h) as literals, and the float64 / float32 evaluations of a row on the CPU.

The dispatch edges the table sits on, for (K, S, pad) = (3,1,1) and (4,2,1):

    forward, weight gradient   4 pixels per thread iff Wo % 4 == 0 and Win % 4 == 0
    data gradient              4 pixels per thread iff Win % 4 == 0, Win >= 8, Hin >= 4 and (K == 3 or Hin even); else the gather

so a 6x4 or 3x8 plane runs the forward on 4 and the data gradient on 1, a 5x16 plane of 4x4/s2 likewise, and 4x8 is the
smallest plane of the border stencil: its folded rows 1 and Hin - 2 are neighbours and one of its two thread columns holds
the left fold, the other the right one.  Reflect padding on a dimension of 3 folds both padded positions onto the middle
index: five (output, tap) pairs in the gather's list (k3-h3, k3-w3, k3-3x3).  (2,2,0) and (6,2,2) always run on 1."""
from typing import NamedTuple, Tuple

import torch

import conv_ref as R
from test_conv_paths_gpu import C_FAMILY, SENTINEL, _gen, _randn
from test_strided_geometry_gpu import C_OP

C = 6            # channels of every row: not a power of two, so a swapped plane % C / plane / C shows


class Row(NamedTuple):
    id: str
    K: int
    S: int
    pad: int
    mode: str                     # "reflect" / "zeros"
    H: int
    W: int
    acc: int                      # a prior gradient on the source (the kernel accumulates)
    paths: Tuple[int, int, int]   # pixels per thread: (forward, data gradient, weight gradient)
    N: int = 3
    padded: Tuple[int, ...] = (1,)
    kind: str = "plain"           # "bias": bname of MBConv; "twice": two calls on one weight in one tape


ROWS = [
    # zero padding on the 3x3 and 4x4 kernels; 40x48: two blocks per plane of the 4-pixel forward and data gradient
    Row("k3-zeros", 3, 1, 1, "zeros", 40, 48, 1, (4, 4, 4)),
    Row("k4-zeros", 4, 2, 1, "zeros", 40, 48, 0, (4, 4, 4)),
    Row("k3-zeros-6x6", 3, 1, 1, "zeros", 6, 6, 1, (1, 1, 1)),
    Row("k4-zeros-6x6", 4, 2, 1, "zeros", 6, 6, 1, (1, 1, 1)),
    # the smallest plane of the border stencil
    Row("k3-min-stencil", 3, 1, 1, "reflect", 4, 8, 1, (4, 4, 4)),
    Row("k3-min-stencil-fresh", 3, 1, 1, "reflect", 4, 8, 0, (4, 4, 4)),
    Row("k4-min-stencil", 4, 2, 1, "reflect", 4, 8, 1, (4, 4, 4)),
    Row("k4-min-stencil-zeros", 4, 2, 1, "zeros", 4, 8, 1, (4, 4, 4)),
    # forward and data gradient on different variants
    Row("k3-w4", 3, 1, 1, "reflect", 6, 4, 0, (4, 1, 4)),
    Row("k3-h3", 3, 1, 1, "reflect", 3, 8, 1, (4, 1, 4)),          # five pairs in the row list
    Row("k3-w3", 3, 1, 1, "reflect", 8, 3, 0, (1, 1, 1)),          # ... in the column list
    Row("k3-3x3", 3, 1, 1, "reflect", 3, 3, 0, (1, 1, 1)),         # ... in both
    Row("k3-3x3-zeros", 3, 1, 1, "zeros", 3, 3, 0, (1, 1, 1)),
    Row("k3-2x2", 3, 1, 1, "reflect", 2, 2, 1, (1, 1, 1)),         # the smallest plane dw_check takes
    Row("k4-odd-h", 4, 2, 1, "reflect", 5, 16, 1, (4, 1, 4)),
    Row("k4-odd-w", 4, 2, 1, "reflect", 8, 9, 0, (1, 1, 1)),       # Wo = 4, Win odd: no float4 spans
    Row("k4-odd-w-zeros", 4, 2, 1, "zeros", 8, 9, 0, (1, 1, 1)),
    # more than 64 frames: lanes 0 and 1 of dw_wgrad_reduce_kernel sum three frames each, (0, 64, 128) and (1, 65, 129)
    Row("k4-n130", 4, 2, 1, "reflect", 8, 8, 1, (4, 4, 4), 130, (1, 64, 65, 129)),
    Row("k6-n70", 6, 2, 2, "reflect", 8, 8, 0, (1, 1, 1), 70, (1, 69)),
    # the bias of MBConv's depthwise convolution (c2s_channel_bias_add with frame flags)
    Row("k3-bias", 3, 1, 1, "reflect", 8, 8, 0, (4, 4, 4), kind="bias"),
    # one weight written twice in a tape: the second weight gradient goes through a temporary and c2s_add_inplace
    Row("k3-weight-twice", 3, 1, 1, "reflect", 8, 8, 0, (4, 4, 4), kind="twice"),
    Row("k4-weight-twice", 4, 2, 1, "reflect", 8, 8, 0, (4, 4, 4), kind="twice"),
]
IDS = [r.id for r in ROWS]

# what the rows must reach together, per geometry: both values of each export, and the mixed triples
REACHED_BOTH = {(3, 1, 1), (4, 2, 1)}
MIXED = {(3, 1, 1): {(4, 1, 4)}, (4, 2, 1): {(4, 1, 4)}}


def constants(row: Row):
    """The per-element constants c of |got - ref64| <= c * u * A the row's kernels are held to."""
    if row.K in (2, 6):
        return dict(C_OP)
    return {"fwd": C_FAMILY["dw"], "dgrad": C_FAMILY["dw"], "wgrad": C_FAMILY["dw_wgrad"]}


def out_hw(row: Row):
    return (row.H + 2 * row.pad - row.K) // row.S + 1, (row.W + 2 * row.pad - row.K) // row.S + 1


def keep_of(row: Row):
    keep = torch.ones(row.N, dtype=torch.bool)
    keep[list(row.padded)] = False
    return keep


def inputs(row: Row):
    """The row's tensors on the CPU, float32: padded frames hold NaN in x and gout and SENTINEL in the prior.  `calls` is a
    list of (x, gout, prior or None): one entry, two for the weight-written-twice rows."""
    g = _gen("dw-" + row.id)
    keep = keep_of(row)
    Ho, Wo = out_hw(row)
    w = torch.randn(C, 1, row.K, row.K, generator=g)
    b = torch.randn(C, generator=g) if row.kind == "bias" else None
    calls = []
    for _ in range(2 if row.kind == "twice" else 1):
        x = _randn((row.N, C, row.H, row.W), g, keep)
        gout = _randn((row.N, C, Ho, Wo), g, keep)
        prior = _randn(x.shape, g, keep, SENTINEL) if row.acc else None
        calls.append((x, gout, prior))
    return {"keep": keep, "w": w, "b": b, "calls": calls}


def evaluate(row: Row, x, w, b, gout, prior, keep, dtype):
    """Forward, data gradient (+ prior) and weight gradient of one call on the real frames, evaluated by torch on the CPU in
    `dtype`: the float32 evaluation is an independent fp32 order of the same sums, to hold against the float64 one."""
    xs = x[keep].detach().clone().to(dtype).requires_grad_(True)
    ws = w.detach().clone().to(dtype).requires_grad_(True)          # (a copy: .to() of the same dtype is w itself)
    y = R._conv(xs, ws, row.S, row.pad, row.mode, C, False)
    if b is not None:
        y = y + b.to(dtype).view(1, -1, 1, 1)
    y.backward(gout[keep].to(dtype))
    gx = xs.grad if prior is None else xs.grad + prior[keep].to(dtype)
    return {"y": y.detach(), "gx": gx, "gw": ws.grad}


def refs(row: Row, x, w, b, gout, prior, keep):
    """float64 results of one call and their bounds A (conv_ref.conv_refs; the prior added as check_conv adds it)."""
    r = R.conv_refs(x[keep], w, b, gout[keep], row.S, row.pad, row.mode, groups=C)
    if prior is not None:
        p = prior[keep].double()
        r["gx"], r["Agx"] = r["gx"] + p, r["Agx"] + p.abs()
    return r


def paths(L, Hin, Win, K, S, pad, mode="reflect"):
    """c2s_dwconv_paths as a triple; `L` is crop2seg_amd._lib.  Raises on a refusal."""
    import ctypes
    f, d, g = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    pm = L.PAD_REFLECT if mode == "reflect" else L.PAD_ZEROS
    rc = L.lib().c2s_dwconv_paths(Hin, Win, K, S, pad, pm, ctypes.byref(f), ctypes.byref(d), ctypes.byref(g))
    assert rc == 0, L.lib().c2s_last_error()
    return f.value, d.value, g.value


def row_paths(L, row: Row):
    return paths(L, row.H, row.W, row.K, row.S, row.pad, row.mode)
