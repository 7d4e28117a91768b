"""The tile walk and the LDS-DMA staging of the 8-wave ring kernels (conv_winograd16.hip, conv_s2wino.hip, conv_s2dgrad.hip;
csrc/conv_ring.h) against the float64 references of tests/conv_ref.py, element by element.

test_conv_paths_gpu.py runs these kernels at N = 3 or 5 frames: a launch has fewer tiles than the one workgroup per compute
unit of the persistent grid, so no workgroup goes on to a second tile and the requests never run across a tile boundary.  Here
N follows the device (walk_frames): every workgroup of the first grid pass multiplies at least three tiles.  The conventions are
those of test_conv_paths_gpu.py: padded frames (valid[n] = 0) hold NaN in x and gout; an accumulated prior gradient holds the
sentinel 1234.5 on the padded frames, which must still be bit-identical after the backward pass; the weight gradient must be
finite; every result meets |got - ref64| <= C_FAMILY[family] * 2^-24 * A element by element and the Frobenius bars of
conv_ref.py.  Every case asserts the families that ran.

Rows, the smallest shapes (K = chunks of the launch; a ring kernel needs K >= 4, conv_s2dgrad K >= 3):

    wino16-walk          3x3 reflect (32,) -> 64 on 16 x 64: four 8 x 32 tiles per frame, forward on wino16 with K = 4.  The data
                         gradient into 32 channels is planned on the implicit GEMM (engine._use_winograd wants 64 output
                         channels), so the walk of the adjoint launch is the next row's
    wino16-walk-dgrad    the same plane, (64,) -> 64: forward K = 8, data gradient on wino16 with the reflect adjoint, K = 8
    wino16-walk-zeros, wino16-walk-dgrad-zeros    the two above zero-padded with a prior: non-adjoint launches, the other
                         `ok` rule of the gather table
    s2-walk              4x4 stride 2 reflect (8,) -> 24 on 32 x 128: forward on s2wino (two 16 x 32 tiles per frame, K = 4,
                         CoutP 64), data gradient on s2dgrad (four 8 x 32 tiles per frame and row parity, K = 3, grid y = 2)
    s2-walk-k5           (10,) -> 40 on the same planes: K = 5 in both

Ring phases at tile starts.  A chunk advances the U ring by two half slabs (mod 5) and the raw ring by one slot (mod 4;
conv_s2dgrad mod 3), so the j-th tile a workgroup multiplies starts at half slab 2 j K mod 5 and raw slot j K mod 4 (3):

    K = 3 (s2dgrad)           half slab 0, 1, 2, 3, 4, ...   raw slot 0 always
    K = 4 (wino16, s2wino)    half slab 0, 3, 1, 4, 2, ...   raw slot 0 always
    K = 5 (s2wino)            half slab 0 always             raw slot 0, 1, 2, 3, ...
    K = 5 (s2dgrad)           half slab 0 always             raw slot 0, 2, 1, ...
    K = 8 (wino16)            half slab 0, 1, 2, 3, 4, ...   raw slot 0 always

and three walked tiles reach the first three entries of each line.

Padded frames (walk_frames): a workgroup that starts in frame k goes on in frames k + F and k + 2 F (F = frames per grid pass
of the launch).  For the F of every ring launch of the row the padded set covers real-padded-real, padded-real-real (four
padded frames in a row among them), real-real-padded and padded-padded-real, and the last frame is padded.

The accumulate 0 / 1 cases of a row share their inputs and their float64 reference (computed once per row).
"""
import math
from typing import Dict

import pytest
import torch

import conv_ref as R
from test_conv_paths_gpu import C_FAMILY, SENTINEL, Row, _ctx, _dgrad_kernel, _fwd_kernel, _gen, _randn

pytestmark = pytest.mark.gpu

RING = ("wino16", "s2wino", "s2dgrad")
# Row of test_conv_paths_gpu (N follows the device; the weight-gradient family is not this file's subject)
ROWS = [
    Row("wino16-walk", 0, (32,), 64, 16, 64, 3, 1, "reflect", (0, 1), "wino16", ("igemm",), -1),
    Row("wino16-walk-dgrad", 0, (64,), 64, 16, 64, 3, 1, "reflect", (0, 1), "wino16", ("wino16",), -1),
    Row("wino16-walk-zeros", 0, (32,), 64, 16, 64, 3, 1, "zeros", (1,), "wino16", ("igemm",), -1),
    Row("wino16-walk-dgrad-zeros", 0, (64,), 64, 16, 64, 3, 1, "zeros", (1,), "wino16", ("wino16",), -1),
    Row("s2-walk", 0, (8,), 24, 32, 128, 4, 2, "reflect", (0, 1), "s2wino", ("s2dgrad",), -1),
    Row("s2-walk-k5", 0, (10,), 40, 32, 128, 4, 2, "reflect", (1,), "s2wino", ("s2dgrad",), -1),
]
CASES = [(row, acc) for row in ROWS for acc in row.acc]       # (here Row.acc lists the accumulate settings to run)


def _cdiv(a, b):
    return -(-a // b)


def ring_passes(row, cus):
    """Frames per grid pass F of every ring-kernel launch of the row: the launchers start ceil(cus / y blocks) workgroups,
    which share a frame's tiles."""
    Ho, Wo = row.H // row.S, row.W // row.S
    launches = []       # (family, tiles per frame, y blocks)
    if row.K == 3:
        tiles = _cdiv(row.H, 8) * _cdiv(row.W, 32)
        launches += [(row.fwd, tiles, _cdiv(row.Cout, 64)), (row.dgrad[0], tiles, _cdiv(row.chans[0], 64))]
    else:
        launches += [(row.fwd, _cdiv(Ho, 16) * _cdiv(Wo, 32), _cdiv(row.Cout, 64)),
                     (row.dgrad[0], _cdiv(Ho, 8) * _cdiv(Wo, 32), 2 * _cdiv(row.chans[0], 64))]
    return sorted({_cdiv(cus, y) // tiles for fam, tiles, y in launches if fam in RING}, reverse=True), launches


def walk_patterns(padded, F):
    """The (frame k, k + F, k + 2 F) padded / real patterns the first three tiles of the workgroups meet"""
    return {tuple(k + j * F in padded for j in range(3)) for k in range(F)}


def walk_frames(row, cus):
    """(N, padded frames) of a row on a device with `cus` compute units: N = 3 F + F // 4 for the largest F of the row's ring
    launches; per F the padded frames that give its workgroups every pattern (module docstring), at start frames of
    their own (base)."""
    Fs, launches = ring_passes(row, cus)
    assert Fs[-1] >= 16 * (len(Fs) - 1) + 11, f"{row.id}: {Fs[-1]} frames per grid pass are too few to place the padded frames"
    N = 3 * Fs[0] + Fs[0] // 4
    padded = {N - 1}
    for i, F in enumerate(Fs):
        b = 16 * i
        padded |= {b + 1, b + 3, b + 4, b + 5, b + 6}       # padded-real-real; four padded frames in a row
        padded |= {b + 8 + F}                               # real-padded-real
        padded |= {b + 9 + 2 * F}                           # real-real-padded
        padded |= {b + 10, b + 10 + F}                      # padded-padded-real
    for fam, tiles, y in launches:
        if fam in RING:
            assert tiles * N >= 3 * _cdiv(cus, y), f"{row.id}: not every {fam} workgroup reaches a third tile"
    want = {(False, True, False), (True, False, False), (False, False, True), (True, True, False)}
    for F in Fs:
        assert want <= walk_patterns(padded, F), f"{row.id}: F = {F} misses {sorted(want - walk_patterns(padded, F))}"
    return N, sorted(padded)


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


SHARED: Dict[str, dict] = {}        # row id -> inputs and float64 reference, shared by the row's cases and left unchanged


def _shared(row):
    if row.id not in SHARED:
        E, _ = _engine()
        N, padded = walk_frames(row, E.lib().c2s_device_cus())
        keep = torch.ones(N, dtype=torch.bool)
        keep[padded] = False
        g = _gen(row.id)
        Cin, K = row.chans[0], row.K
        x = _randn((N, Cin, row.H, row.W), g, keep)
        w = torch.randn(row.Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
        b = torch.randn(row.Cout, generator=g)
        gout = _randn((N, row.Cout, row.H // row.S, row.W // row.S), g, keep)
        prior = _randn(x.shape, g, keep, SENTINEL)
        ref = R.conv_refs(x[keep], w, b, gout[keep], row.S, 1, row.mode, weight_grad=False)
        SHARED[row.id] = dict(N=N, keep=keep, x=x, w=w, b=b, gout=gout, prior=prior, ref=ref)
    return SHARED[row.id]


@pytest.mark.parametrize("row,acc", CASES, ids=[f"{r.id}-acc{a}" for r, a in CASES])
def test_conv_walk(row, acc):
    E, L = _engine()
    s = _shared(row)
    keep, ref = s["keep"], s["ref"]
    pm = L.PAD_REFLECT if row.mode == "reflect" else L.PAD_ZEROS
    ctx = _ctx({"w": s["w"], "b": s["b"]})
    xd = s["x"].cuda()
    if acc:
        ctx.tape.grads[xd.data_ptr()] = s["prior"].cuda()
    out = E.conv2d(ctx, [xd], "w", "b", row.K, row.S, 1, pm, keep.int().cuda())
    ctx.tape.grads[out.data_ptr()] = s["gout"].cuda()
    ctx.tape.backward()
    torch.cuda.synchronize()
    fwd, dgrad = _fwd_kernel(ctx), _dgrad_kernel(ctx, 0)
    assert (fwd, dgrad) == (row.fwd, row.dgrad[0]), f"{row.id}: reached {fwd} / {dgrad}, the table says {row.fwd} / {row.dgrad[0]}"

    q_fwd = R.assert_within("forward", out.cpu()[keep], ref["y"], ref["Ay"], C_FAMILY[fwd], R.FROB_FWD)
    got = ctx.tape.grads[xd.data_ptr()].cpu()
    p = s["prior"][keep].double() if acc else torch.zeros((), dtype=torch.float64)
    q_dgrad = R.assert_within("data gradient", got[keep], ref["gx"] + p, ref["Agx"] + p.abs(), C_FAMILY[dgrad], R.FROB_GRAD)
    if acc:
        same = got[~keep].view(torch.int32) == s["prior"][~keep].view(torch.int32)
        assert bool((s["prior"][~keep] == SENTINEL).all()) and bool(same.all()), \
            f"{row.id}: padded-frame gradient overwritten: {int((~same).sum())} elements"
    assert bool(torch.isfinite(ctx.g["w"]).all()), f"{row.id}: weight gradient not finite (a kernel read a padded frame?)"
    print(f"\n{row.id} acc {acc}: N {s['N']}  fwd {fwd} {q_fwd:.2f}  dgrad {dgrad} {q_dgrad:.2f}")
