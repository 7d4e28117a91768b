"""Convolution kernels on non-square planes against the float64 references of tests/conv_ref.py.

Every kernel family is picked from H and W separately (engine._use_winograd, _wide_winograd, the *_supported predicates of
the library), and a square plane reaches a family only where both sides pass: the tables of test_conv_paths_gpu.py and
test_strided_geometry_gpu.py run H == W (or near it) throughout, so a swapped H / W in a descriptor, a tile loop or the
reflect fold would pass them.  The rows here are the (family, plane) cells rectangles reach through the ordinary model path
and squares never do: the 4-wave Winograd kernel at H = 2 and 4, on W >= 32 with H < 8, and on tall planes 8 and 16 wide;
the 8-wave kernel at its smallest plane; the implicit GEMM on tall thin planes; the 4x4 stride-2 convolution refused by the
F(2x2,2x2) kernels on its height alone; conv_xpair and the transposed convolutions (K = 4, 2, 6) on H != W, W = 2 included;
and planes 3 pixels wide or high, where both reflected rows of the data gradient fold onto position 1.

Method of test_conv_paths_gpu._run_row (reused, with its REACHED / REACHED_WGRAD / OBSERVED records put back afterwards, so
that file's test_reached_paths_are_the_table still sees its own table only): N = 3 with frame 1 padded and NaN in x and
gout, accumulating rows carry a prior and the 1234.5 sentinel on the padded frame, every element meets
|got - ref64| <= c * u * A, and each row asserts the forward, data-gradient and weight-gradient family it reached.  The
weight-gradient literals are read off the table in include/c2s_hip.h (a gout plane of whole 4 x 32 tiles with >= 32 channels
both ways: 4 / 5 for 3x3, 6 for 4x4 stride 2; else a multiple of 32 wide and even in height: 1; 16 wide and a multiple of
4 high: 2; anything else, K = 2 and K = 6 included: the generic 0) and held against c2s_wgrad_path; tests/test_conv_plan_rect.py
holds the same table against the plan without a GPU.  Constants: C_FAMILY of test_conv_paths_gpu.py with one entry moved by
that file's rule (C_RECT below, with the observation), C_OP of test_strided_geometry_gpu.py for the parity geometries
(K = 2, 6) down and up; the K = 4 transposed rows keep the tighter family constants of test_conv_paths_gpu._run_transpose.

Observed worst ratios max |err| / (u * A) on an MI355X (printed with -s by test_worst_ratios):

    wino16 2.19   wino4 2.34   igemm 4.25   s2wino 4.48   s2dgrad 4.85   xpair 5.21
    wgrad_direct 3.44   wgrad_f23 2.21   wgrad_f22 2.25 (conv2d rows) / 2.67 (transposed 4 x 32)
    K = 2, 6 down: fwd 4.61  dgrad 4.96  wgrad 3.21        K = 2, 6 up: fwd 4.22  dgrad 4.07  wgrad 3.02
    K = 4 up: fwd (xpair) 4.22  dgrad (igemm) 5.11  wgrad_direct 3.22

Found by these rows: the 3-pixel planes were refused by conv_igemm.hip in the middle of the backward pass ("reflect_adjoint
needs planes of 2 or >= 4"); the kernel's two border rules sit on different taps of position 1 and both apply, so the
refusal is gone and ROWS_3PX hold the result.  Nothing else: every rectangle row passed as the kernels stood.

The rows can fail: with engine.conv_transpose2d's forward planned on the transposed plane (conv_plan("tfwd") called with
Hin and Win swapped: a local patch, not part of the project; every launch stays inside its tensors), all 24 rows of
test_conv_transpose_rect fail here, while test_conv_paths_gpu.py, test_strided_geometry_gpu.py (its three whole models
included) and the older cases of test_redzone_gpu.py all still pass.
"""
import math

import pytest
import torch

import conv_ref as R
import test_conv_paths_gpu as P
from test_conv_paths_gpu import Row
from test_strided_geometry_gpu import C_OP, GEOMS

pytestmark = pytest.mark.gpu

OBSERVED = {}           # family -> worst ratio over the rows of this file that ran
# C_FAMILY with one constant moved, by the rule of test_conv_paths_gpu.py (about 4x the worst ratio observed on an MI355X over
# the family's rows, capped at 1024).  wgrad_f22, the F(2x2,2x2) weight gradient: 2 there, from 0.47 observed on its rows,
# which sum 2 x 64 x 64 positions into every element.  Its transforms take differences of neighbouring pixels, so a term's
# rounding error is a few u times the term whatever the plane, while the errors of P terms add up like sqrt(P) against an
# A that grows like P: the ratio falls with the plane.  Here the smallest plane the family takes, one 4 x 32 tile per frame
# (256 positions), gives 2.67, 2.60, 2.25, 2.09 on its four rows and the 8 x 32 row 1.35 (1 ... 13 of 65536 elements beyond
# c = 2, none beyond 2.7; an indexing fault lands near 1e7).  4 x 2.67 = 10.7.
C_RECT = {**P.C_FAMILY, "wgrad_f22": 11}


def _note(family, ratio):
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), ratio)


def _r(id_, chans, Cout, H, W, K, S, mode, acc, fwd, dgrad, wgrad):
    return Row("rect-" + id_, 3, chans, Cout, H, W, K, S, mode, acc, fwd, dgrad, wgrad)


ROWS = [
    # 4-wave Winograd: H = 2 (level 3 of a 16 x 64 input); W >= 32 with H < 8 (the 8-wave kernel refuses on height alone);
    # tall planes 8 and 16 wide
    _r("wino4-2x8", (128,), 128, 2, 8, 3, 1, "reflect", (0,), "wino4", ("wino4",), 0),
    _r("wino4-2x8-acc", (128,), 128, 2, 8, 3, 1, "reflect", (1,), "wino4", ("wino4",), 0),
    _r("wino4-4x32-acc", (64,), 64, 4, 32, 3, 1, "reflect", (1,), "wino4", ("wino4",), 5),
    _r("wino4-2x64-acc", (64,), 64, 2, 64, 3, 1, "reflect", (1,), "wino4", ("wino4",), 1),
    _r("wino4-64x8-acc", (64,), 64, 64, 8, 3, 1, "reflect", (1,), "wino4", ("wino4",), 0),
    _r("wino4-32x16", (64,), 64, 32, 16, 3, 1, "reflect", (0,), "wino4", ("wino4",), 2),
    # two sources: 64 output channels into the 32-channel source run on the implicit GEMM (Winograd needs cout >= 64)
    _r("wino4-two-sources-4x32-acc-skip", (32, 64), 64, 4, 32, 3, 1, "reflect", (0, 1), "wino4", ("igemm", "wino4"), 4),
    # 8-wave Winograd at the smallest plane its predicate takes, and twice as wide
    _r("wino16-8x32-acc", (64,), 64, 8, 32, 3, 1, "reflect", (1,), "wino16", ("wino16",), 5),
    _r("wino16-8x64", (64,), 64, 8, 64, 3, 1, "reflect", (0,), "wino16", ("wino16",), 5),
    # implicit GEMM 3x3 on tall thin planes (W < 8) and 2 x 4
    _r("igemm-16x4-acc", (64,), 64, 16, 4, 3, 1, "reflect", (1,), "igemm", ("igemm",), 0),
    _r("igemm-8x2", (128,), 128, 8, 2, 3, 1, "reflect", (0,), "igemm", ("igemm",), 0),
    _r("igemm-8x2-acc", (128,), 128, 8, 2, 3, 1, "reflect", (1,), "igemm", ("igemm",), 0),
    _r("igemm-2x4", (128,), 128, 2, 4, 3, 1, "reflect", (0,), "igemm", ("igemm",), 0),
    _r("igemm-2x4-acc", (128,), 128, 2, 4, 3, 1, "reflect", (1,), "igemm", ("igemm",), 0),
    # Cout < 64: implicit-GEMM forward; its data gradient (32 -> 64 channels) is a 4-wave Winograd launch on 4 x 32
    _r("igemm-cout32-4x32-acc", (64,), 32, 4, 32, 3, 1, "reflect", (1,), "igemm", ("wino4",), 5),
    _r("igemm-cout32-4x32-zeros-acc", (64,), 32, 4, 32, 3, 1, "zeros", (1,), "igemm", ("wino4",), 5),
    # 4x4 stride 2: 8 x 64 -> 4 x 32 is wide enough for the F(2x2,2x2) kernels and refused on its height
    _r("s2-8x64-igemm-xpair-acc", (64,), 64, 8, 64, 4, 2, "reflect", (1,), "igemm", ("xpair",), 6),
    _r("s2-8x64-igemm-xpair", (64,), 64, 8, 64, 4, 2, "reflect", (0,), "igemm", ("xpair",), 6),
    _r("xpair-8x32-acc", (64,), 64, 8, 32, 4, 2, "reflect", (1,), "igemm", ("xpair",), 2),
    _r("xpair-8x32", (64,), 64, 8, 32, 4, 2, "reflect", (0,), "igemm", ("xpair",), 2),
    _r("xpair-32x8-acc", (64,), 64, 32, 8, 4, 2, "reflect", (1,), "igemm", ("xpair",), 0),
    _r("xpair-32x8", (64,), 64, 32, 8, 4, 2, "reflect", (0,), "igemm", ("xpair",), 0),
    _r("xpair-4x16-acc", (64,), 64, 4, 16, 4, 2, "reflect", (1,), "igemm", ("xpair",), 0),
    _r("xpair-4x16", (64,), 64, 4, 16, 4, 2, "reflect", (0,), "igemm", ("xpair",), 0),
    _r("xpair-16x4-acc", (64,), 64, 16, 4, 4, 2, "reflect", (1,), "igemm", ("xpair",), 0),
    _r("xpair-16x4", (64,), 64, 16, 4, 4, 2, "reflect", (0,), "igemm", ("xpair",), 0),
    # ... and the F(2x2,2x2) kernels at their minimum, 16 x 64 -> 8 x 32
    _r("s2wino-16x64-acc", (64,), 64, 16, 64, 4, 2, "reflect", (1,), "s2wino", ("s2dgrad",), 6),
]

# planes 3 pixels wide or high (level 3 of a 24-pixel side): lo == hi == 1 in the reflect fold of the data gradient
ROWS_3PX = [_r(f"3px-{c}ch-{H}x{W}{'-acc' if a else ''}", (c,), c, H, W, 3, 1, "reflect", (a,), "igemm", ("igemm",), 0)
            for c in (64, 128) for H, W in ((3, 8), (8, 3), (3, 3)) for a in (0, 1)]


def _run(row):
    """test_conv_paths_gpu._run_row under C_RECT, with that module's records and constants put back: the rows of this file are
    not part of its table."""
    saved, saved_c = dict(P.OBSERVED), dict(P.C_FAMILY)
    P.OBSERVED.clear()
    P.C_FAMILY.update(C_RECT)
    try:
        P._run_row(row)
    finally:
        mine = dict(P.OBSERVED)
        P.OBSERVED.clear()
        P.OBSERVED.update(saved)
        P.C_FAMILY.clear()
        P.C_FAMILY.update(saved_c)
        P.REACHED.pop(row.id, None)
        P.REACHED_WGRAD.pop(row.id, None)
    for k, v in mine.items():
        _note(k, v)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_conv2d_rect(row):
    _run(row)


@pytest.mark.parametrize("row", ROWS_3PX, ids=[r.id for r in ROWS_3PX])
def test_conv2d_three_pixel_plane(row):
    _run(row)


# =================================================================================================
# parity geometries (K, pad) = (2, 0) and (6, 2): down convolution
# =================================================================================================
DOWN = [(K, p, mode, H, W, acc) for K, p in GEOMS for mode in ("reflect", "zeros") for H, W in ((8, 32), (32, 8))
        for acc in (0, 1)]


@pytest.mark.parametrize("K,pad,mode,H,W,acc", DOWN)
def test_down_conv_rect(K, pad, mode, H, W, acc):
    E, L = P._engine()
    N, cin, cout = 3, 64, 64
    g = P._gen(f"rect-down{K}{pad}{mode}{H}{W}{acc}")
    keep = P._keep(N)
    pm = L.PAD_REFLECT if mode == "reflect" else L.PAD_ZEROS
    Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
    x = P._randn((N, cin, H, W), g, keep)
    w = torch.randn(cout, cin, K, K, generator=g) / math.sqrt(cin * K * K)
    b = torch.randn(cout, generator=g)
    gout = P._randn((N, cout, Ho, Wo), g, keep)
    ctx = P._ctx({"w": w, "b": b})
    xd = x.cuda()
    prior, sentinel = None, None
    if acc:
        prior = P._randn(x.shape, g, keep, P.SENTINEL)
        sentinel = (~keep).view(N, 1, 1, 1).expand(x.shape).clone()
        ctx.tape.grads[xd.data_ptr()] = prior.cuda()
    out = E.conv2d(ctx, [xd], "w", "b", K, 2, pad, pm, keep.int().cuda())
    assert out.shape == (N, cout, H // 2, W // 2)
    ctx.tape.grads[out.data_ptr()] = gout.cuda()
    ctx.tape.backward()
    torch.cuda.synchronize()
    # implicit GEMM forward, four parity launches of the data gradient, the generic weight-gradient kernel (K = 2, 6)
    assert ("w", "fwd") in ctx._packed and ("w", "fwd", "s2w") not in ctx._packed
    assert all(("w", "dgrad", 0, "par", py, px) in ctx._packed for py in range(2) for px in range(2))
    assert P.wgrad_family(ctx, [xd], cout, Ho, Wo, K, 2, pad, pm) == 0
    ratios = R.check_conv(out.cpu(), ctx.tape.grads[xd.data_ptr()].cpu(), ctx.g["w"].cpu(), x, w, b, gout, keep, 2, pad,
                          mode, C_OP, prior=prior, sentinel=sentinel)
    _note("parity_fwd", ratios["fwd"])
    _note("parity_dgrad", ratios["dgrad"])
    _note("parity_wgrad", ratios["wgrad"])
    print(f"\ndown k{K} p{pad} {mode} {H}x{W} acc={acc}: {ratios}")


# =================================================================================================
# transposed convolution, K = 4, 2, 6
# =================================================================================================
UP_SHAPES = [(128, 64, 2, 8), (128, 64, 8, 2), (64, 32, 4, 32), (64, 16, 16, 4)]
# weight gradient = convKxKs2 wgrad with (input = gout, gout = x): gout-channels -> Cin channels on the H x W plane.  K = 4:
# 4 x 32 with 32 -> 64 channels tiles into 4 x 32 (F(2x2,2x2), 6); the other planes are neither 16 nor a multiple of 32 wide
UP_WGRAD = {(4, 4, 32): 6}
UP = [(K, p, cin, cout, H, W, acc) for K, p in [(4, 1)] + GEOMS for cin, cout, H, W in UP_SHAPES for acc in (0, 1)]


@pytest.mark.parametrize("K,pad,cin,cout,H,W,acc", UP)
def test_conv_transpose_rect(K, pad, cin, cout, H, W, acc):
    E, L = P._engine()
    N = 2
    g = P._gen(f"rect-up{K}{pad}{cin}{cout}{H}{W}{acc}")
    keep = torch.ones(N, dtype=torch.bool)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cin, cout, K, K, generator=g) / math.sqrt(cin * K)
    b = torch.randn(cout, generator=g)
    gout = torch.randn(N, cout, 2 * H, 2 * W, generator=g)
    ctx = P._ctx({"w": w, "b": b})
    xd = x.cuda()
    prior = None
    if acc:
        prior = torch.randn(x.shape, generator=g)
        ctx.tape.grads[xd.data_ptr()] = prior.cuda()
    out = E.conv_transpose2d(ctx, xd, "w", "b", K, pad)
    assert out.shape == (N, cout, 2 * H, 2 * W)
    gd = gout.cuda()
    ctx.tape.grads[out.data_ptr()] = gd
    ctx.tape.backward()
    torch.cuda.synchronize()
    assert ("w", "dgrad") in ctx._packed                                                   # conv_igemm<K, 2>
    if K == 4:
        assert ("w", "fwd", 0) in ctx._packed and ("w", "fwd", 1) in ctx._packed           # conv_xpair, one launch per row parity
        assert not any("par" in k for k in ctx._packed)
    else:
        assert all(("w", "fwd", "par", py, px) in ctx._packed for py in range(2) for px in range(2))
    fam = UP_WGRAD.get((K, H, W), 0)
    wk = P._observed_wgrad(ctx, [gd], xd, cin, H, W, K, 2, pad, L.PAD_ZEROS, cout * K * K, K * K, list(range(K * K)), None,
                           ctx.g["w"])
    P._check_wgrad(f"up k{K} {H}x{W}", ctx, [gd], cin, H, W, K, 2, pad, L.PAD_ZEROS, wk, fam)
    c = {"fwd": C_RECT["xpair"], "dgrad": C_RECT["igemm"], "wgrad": C_RECT[wk]} if K == 4 else C_OP
    ratios = R.check_conv(out.cpu(), ctx.tape.grads[xd.data_ptr()].cpu(), ctx.g["w"].cpu(), x, w, b, gout, keep, 2, pad,
                          "zeros", c, prior=prior, transpose=True)
    tag = "up4" if K == 4 else "up_parity"
    _note(f"{tag}_fwd", ratios["fwd"])
    _note(f"{tag}_dgrad", ratios["dgrad"])
    _note(f"{tag}_{wk}", ratios["wgrad"])
    print(f"\nup k{K} p{pad} {cin}->{cout} {H}x{W} acc={acc}: {ratios}")


def test_worst_ratios():
    """The record for the docstring: worst |err| / (u * A) per kernel family over the rows of this file that ran."""
    print("\nworst |err| / (u * A) per kernel family: " + "  ".join(f"{k} {v:.2f}" for k, v in sorted(OBSERVED.items())))
