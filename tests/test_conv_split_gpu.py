"""Split tiles of c2s_conv_igemm (C2S_IGEMM_SPLIT = 1, 2, 4) against the float64 references of tests/conv_ref.py, through
engine.conv2d / conv_transpose2d as tests/test_conv_paths_gpu.py drives them.

Per case and forced split: forward, data gradient and weight gradient meet |got - ref64| <= c * u * A element by element
with the family constants of test_conv_paths_gpu.py (c = 20 for igemm and xpair; the weight-gradient kernels are not part
of the split and keep the constant of the family c2s_wgrad_path reports) and the Frobenius bars FROB_FWD / FROB_GRAD; the
same call run twice is bit-identical; a padded frame (valid = 0, NaN content) is never read and, where a prior gradient
sits on the source, its sentinel 1234.5 is bit-identical afterwards.  nn.ConvTranspose2d takes no frame flags in the
engine, so its cases run three real frames.  The observed ratios are printed with -s.

The split divides the positions of a tile over more workgroups and leaves every output element its chain of MFMAs, so
the results of split 2 and 4 are also bit-identical to split 1 (test_splits_are_bit_identical):
the observed ratios are those of the unsplit kernel, 5.01 at the worst over these cases.  c2s_conv_xpair has no split
(its K-split form was measured and not kept); its rows stay because the implicit-GEMM launches next to them are
cases of the table (the K = 4, S = 2 forward and the data gradient of the transposed convolution).
"""
import ctypes
import functools
import math
import zlib
from typing import NamedTuple, Tuple

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
C_SPLIT = 20                                    # igemm and xpair (C_FAMILY of test_conv_paths_gpu.py)
C_WGRAD = (12,) * 4 + (4,) * 2 + (2,)           # per c2s_wgrad_path family: wgrad_direct x 4, wgrad_f23 x 2, wgrad_f22
PAD = {1: 0, 2: 0, 3: 1, 4: 1, 6: 2}


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _ctx(params):
    E, _ = _engine()
    dev = torch.device("cuda")
    p = {k: v.to(dev).contiguous() for k, v in params.items()}
    g = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    return E.Ctx(p, {}, g, E.Workspace(dev), True, E.Tape())


def _randn(shape, g, keep=None, pad_value=float("nan")):
    t = torch.randn(shape, generator=g)
    if keep is not None:
        t[~keep] = pad_value
    return t


class Case(NamedTuple):
    id: str
    op: str                       # "conv" (engine.conv2d) or "tconv" (engine.conv_transpose2d)
    chans: Tuple[int, ...]
    Cout: int
    H: int
    W: int
    K: int
    S: int
    mode: str
    acc: Tuple[int, ...]          # per source: prior gradient on the tape
    dgrad: str                    # data-gradient kernel: "igemm", "xpair" or "parity" (four igemm launches)


CASES = [
    # one chunk (the shortest K loop a 3x3 layer has), log2fc = 3
    Case("3x3-cin4-8x8", "conv", (4,), 32, 8, 8, 3, 1, "reflect", (0,), "igemm"),
    # three chunks, ragged Cout, log2fc = 4
    Case("3x3-cin12-cout15-16x16", "conv", (12,), 15, 16, 16, 3, 1, "reflect", (0,), "igemm"),
    # ragged plane, tile overhang both ways, log2fc = 5
    Case("3x3-cin36-20x36", "conv", (36,), 32, 20, 36, 3, 1, "reflect", (0,), "igemm"),
    # two sources, data gradient into each, without and with a prior gradient
    Case("3x3-two-sources", "conv", (16, 8), 32, 32, 32, 3, 1, "reflect", (0, 0), "igemm"),
    Case("3x3-two-sources-acc", "conv", (16, 8), 32, 32, 32, 3, 1, "reflect", (1, 1), "igemm"),
    # tiny plane
    Case("3x3-128ch-4x4", "conv", (128,), 128, 4, 4, 3, 1, "reflect", (0,), "igemm"),
    # K = 1, CK = 16
    Case("1x1-cin64-16x16", "conv", (64,), 32, 16, 16, 1, 1, "zeros", (1,), "igemm"),
    # transposed convolution 32 -> 16, 8x8 -> 16x16: its data gradient is the K = 4, S = 2 launch 16 -> 32, 16x16 -> 8x8
    Case("tconv-dgrad-4x4s2", "tconv", (32,), 16, 8, 8, 4, 2, "zeros", (1,), "igemm"),
    # 4x4 stride 2 with few channels: igemm forward, xpair data gradient with the reflect adjoint
    Case("4x4s2-cin8-8x8", "conv", (8,), 32, 8, 8, 4, 2, "reflect", (0,), "xpair"),
    Case("4x4s2-cin8-8x8-acc", "conv", (8,), 32, 8, 8, 4, 2, "reflect", (1,), "xpair"),
    # nn.ConvTranspose2d(4, 2, 1) 32 -> 32, 8x8 -> 16x16: xpair forward, both row parities
    Case("tconv-xpair-fwd", "tconv", (32,), 32, 8, 8, 4, 2, "zeros", (0,), "igemm"),
    # PARITY_GEOMETRIES: output placement osy = osx = 2 with ooy / oox, reflect_adjoint = 2 (K = 6)
    Case("6x6s2-8x8", "conv", (16,), 32, 8, 8, 6, 2, "reflect", (1,), "parity"),
    Case("2x2s2-8x8", "conv", (16,), 32, 8, 8, 2, 2, "zeros", (0,), "parity"),
]


@functools.lru_cache(maxsize=None)
def _data(case: Case):
    """Inputs and float64 references of a case, computed once and shared by its forced splits (never modified)."""
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    N, K, S, pad = 3, case.K, case.S, PAD[case.K]
    Cin = sum(case.chans)
    keep = torch.ones(N, dtype=torch.bool)
    if case.op == "conv":
        keep[1] = False
        Ho, Wo = (case.H + 2 * pad - K) // S + 1, (case.W + 2 * pad - K) // S + 1
        w = torch.randn(case.Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
    else:
        Ho, Wo = 2 * case.H, 2 * case.W
        w = torch.randn(Cin, case.Cout, K, K, generator=g) / math.sqrt(Cin * K)
    x = _randn((N, Cin, case.H, case.W), g, keep)
    b = torch.randn(case.Cout, generator=g)
    gout = _randn((N, case.Cout, Ho, Wo), g, keep)
    prior = torch.zeros_like(x)
    sentinel = torch.zeros(x.shape, dtype=torch.bool)
    lo = 0
    for c, a in zip(case.chans, case.acc):
        if a:
            prior[:, lo:lo + c] = _randn((N, c, case.H, case.W), g, keep, SENTINEL)
            sentinel[~keep, lo:lo + c] = True
        lo += c
    ref = R.conv_refs(x[keep], w, b, gout[keep], S, pad, case.mode, transpose=case.op == "tconv")
    return dict(x=x, w=w, b=b, gout=gout, keep=keep, prior=prior, sentinel=sentinel, ref=ref, Ho=Ho, Wo=Wo)


def _run(case: Case, d):
    """One forward + backward pass of the case; returns (out, gx, gw, weight-gradient family) on the CPU."""
    E, L = _engine()
    K, S, pad = case.K, case.S, PAD[case.K]
    pm = L.PAD_REFLECT if case.mode == "reflect" else L.PAD_ZEROS
    ctx = _ctx({"w": d["w"], "b": d["b"]})
    srcs, lo = [], 0
    for c, a in zip(case.chans, case.acc):
        srcs.append(d["x"][:, lo:lo + c].contiguous().cuda())
        if a:
            ctx.tape.grads[srcs[-1].data_ptr()] = d["prior"][:, lo:lo + c].contiguous().cuda()
        lo += c
    gd = d["gout"].cuda()
    pk = ctx._packed
    if case.op == "conv":
        vd = d["keep"].int().cuda()
        out = E.conv2d(ctx, srcs, "w", "b", K, S, pad, pm, vd)
        fam = ctypes.c_int(-1)
        assert E.lib().c2s_wgrad_path(ctypes.byref(E._wgrad_desc(ctx, srcs, case.Cout, d["Ho"], d["Wo"], K, S, pad, pm)),
                                      ctypes.byref(fam)) == 0
    else:
        out = E.conv_transpose2d(ctx, srcs[0], "w", "b", K, pad)
        fam = ctypes.c_int(-1)
        assert E.lib().c2s_wgrad_path(ctypes.byref(E._wgrad_desc(ctx, [gd], sum(case.chans), case.H, case.W, K, 2, pad,
                                                                 L.PAD_ZEROS)), ctypes.byref(fam)) == 0
    ctx.tape.grads[out.data_ptr()] = gd
    ctx.tape.backward()
    torch.cuda.synchronize()
    # the kernels the case is about were the ones launched
    if case.op == "conv":
        assert ("w", "fwd") in pk and not any(k[:3] in (("w", "fwd", "wino"), ("w", "fwd", "s2w")) for k in pk), list(pk)
        for si in range(len(srcs)):
            if case.dgrad == "igemm":
                assert ("w", "dgrad", si) in pk, list(pk)
            elif case.dgrad == "xpair":
                assert ("w", "dgrad", si, 0) in pk and ("w", "dgrad", si, 1) in pk, list(pk)
            else:
                assert all(("w", "dgrad", si, "par", py, px) in pk for py in range(2) for px in range(2)), list(pk)
    else:
        assert ("w", "fwd", 0) in pk and ("w", "fwd", 1) in pk and ("w", "dgrad") in pk, list(pk)
    gx = torch.cat([ctx.tape.grads[s.data_ptr()].cpu() for s in srcs], 1)
    return out.cpu(), gx, ctx.g["w"].cpu(), fam.value


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("sp", [1, 2, 4])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_forced_split(case, sp, monkeypatch):
    """Forward, data gradient and weight gradient of a case under a forced split, run twice."""
    monkeypatch.setenv("C2S_IGEMM_SPLIT", str(sp))
    d = _data(case)
    keep, ref = d["keep"], d["ref"]
    out, gx, gw, fam = _run(case, d)
    out2, gx2, gw2, _ = _run(case, d)
    assert _bits_equal(out[keep], out2[keep]) and _bits_equal(gx[keep], gx2[keep]) and _bits_equal(gw, gw2), \
        "the same call run twice is not bit-identical"
    p = d["prior"][keep].double()
    ratios = {
        "fwd": R.assert_within("forward", out[keep], ref["y"], ref["Ay"], C_SPLIT, R.FROB_FWD),
        "dgrad": R.assert_within("data gradient", gx[keep], ref["gx"] + p, ref["Agx"] + p.abs(), C_SPLIT, R.FROB_GRAD),
        "wgrad": R.assert_within("weight gradient", gw, ref["gw"], ref["Agw"], C_WGRAD[fam], R.FROB_GRAD),
    }
    print(f"\n{case.id} split={sp}: fwd {ratios['fwd']:.2f}  dgrad {ratios['dgrad']:.2f}  wgrad(family {fam}) {ratios['wgrad']:.2f}")
    if bool(d["sentinel"].any()):
        same = gx[d["sentinel"]].view(torch.int32) == d["prior"][d["sentinel"]].view(torch.int32)
        assert bool(same.all()), f"padded-frame gradient overwritten: {int((~same).sum())} elements"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_splits_are_bit_identical(case, monkeypatch):
    """Split 2 and 4 give the bits of split 1: forward, data gradient and weight gradient."""
    d = _data(case)
    keep = d["keep"]
    got = {}
    for sp in (1, 2, 4):
        monkeypatch.setenv("C2S_IGEMM_SPLIT", str(sp))
        got[sp] = _run(case, d)
    for sp in (2, 4):
        assert _bits_equal(got[sp][0][keep], got[1][0][keep]), f"forward at split {sp}"
        assert _bits_equal(got[sp][1][keep], got[1][1][keep]), f"data gradient at split {sp}"
        assert _bits_equal(got[sp][2], got[1][2]), f"weight gradient at split {sp}"


def test_split_1_is_the_unsplit_kernel(monkeypatch):
    """Where the rule picks 1 (3x3 32 -> 32 at 128x128, N = 8: 512 workgroups on 256 CUs), forcing 1 changes nothing:
    bit-identical forward and data gradient."""
    E, L = _engine()
    d = L.ConvDesc(8, 32, 0, 128, 128, 32, 32, 128, 128, 128, 128, 3, 3, 1, 1, 1, L.PAD_REFLECT, 1, 1, 0, 0, 0, 0)
    assert E.lib().c2s_conv_igemm_split(ctypes.byref(d), 0) == 1

    def run():
        g = torch.Generator().manual_seed(7)
        x = torch.randn(8, 32, 128, 128, generator=g)
        w = torch.randn(32, 32, 3, 3, generator=g) / math.sqrt(32 * 9)
        ctx = _ctx({"w": w})
        xd = x.cuda()
        out = E.conv2d(ctx, [xd], "w", None, 3, 1, 1, L.PAD_REFLECT, None)
        ctx.tape.grads[out.data_ptr()] = torch.randn(out.shape, generator=g).cuda()
        ctx.tape.backward()
        torch.cuda.synchronize()
        assert ("w", "fwd") in ctx._packed and ("w", "dgrad", 0) in ctx._packed
        return out.cpu(), ctx.tape.grads[xd.data_ptr()].cpu()

    monkeypatch.delenv("C2S_IGEMM_SPLIT", raising=False)
    y0, g0 = run()
    monkeypatch.setenv("C2S_IGEMM_SPLIT", "1")
    y1, g1 = run()
    assert _bits_equal(y0, y1) and _bits_equal(g0, g1)
