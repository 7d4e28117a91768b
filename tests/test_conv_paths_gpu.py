"""Accumulate and padded-frame paths of every convolution kernel against the float64 references of tests/conv_ref.py.

The op tests (test_ops_gpu.py) start every backward pass with an empty tape, so the data-gradient kernels only run with
accumulate = 0 there, and padded frames hold finite numbers.  Here:

- frames: N >= 3 with padded frames (valid[n] = 0) whose x and gout are NaN: a kernel that reads a padded frame turns a
  real output or the weight gradient into NaN;
- accumulating rows pre-seed the tape with a prior gradient on the source: finite random numbers on the real frames and
  the sentinel 1234.5 on the padded frames, which must still be bit-identical after the backward pass;
- every result meets |got - ref64| <= c * u * A element by element (u = 2^-24, A = the same map on absolute values) and
  the Frobenius bars of test_ops_gpu.py (2e-6 forward, 5e-6 gradients);
- every row asserts the kernels it reached, and test_reached_paths_are_the_table asserts the whole set.  The weight-gradient
  kernel is the family c2s_wgrad_path reports (the table in include/c2s_hip.h) against the row's literal, and the class of
  that family (WGRAD_CLASS) against the one observed from bit-identity with the forced runs.

Error constants c per kernel family: about 4x the worst ratio max |err| / (u * A) observed over the rows of the family on
an MI355X (printed with -s), capped at 1024; an indexing or accumulation bug lands near 1/u ~ 1e7.  Observed worst ratios:

    wino16 2.68   wino4 2.17   igemm 4.53   s2wino 4.93   s2dgrad 7.68   xpair 4.67   dw 3.88
    wgrad_direct 2.58   wgrad_f23 0.72   wgrad_f22 0.47   dw_wgrad 1.57

The rows can fail: with the 8-wave Winograd epilogue changed to skip the accumulate add for mt == 1 (a local build, not
part of the project), the five rows that accumulate through that kernel fail here while every convolution test of
test_ops_gpu.py still passes.
"""
import ctypes
import math
import zlib
from typing import NamedTuple, Tuple

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
C_FAMILY = {
    "wino16": 12, "wino4": 10, "igemm": 20, "s2wino": 20, "s2dgrad": 32, "xpair": 20, "dw": 16,
    "wgrad_direct": 12, "wgrad_f23": 4, "wgrad_f22": 2, "dw_wgrad": 8,
}
OBSERVED = {}           # family -> worst ratio over the rows that ran
REACHED = {}            # row id -> set of (kernel, accumulate, reflect_adjoint)
REACHED_WGRAD = {}      # row id -> set of weight-gradient families (c2s_wgrad_path)
# class of a c2s_wgrad_path family: which algorithm it evaluates, hence how it rounds (keys of C_FAMILY)
WGRAD_CLASS = ("wgrad_direct",) * 4 + ("wgrad_f23",) * 2 + ("wgrad_f22",)


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


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _keep(N):
    keep = torch.ones(N, dtype=torch.bool)
    keep[1] = False
    if N >= 5:
        keep[3] = False
    return keep


def _randn(shape, g, keep=None, pad_value=float("nan")):
    t = torch.randn(shape, generator=g)
    if keep is not None:
        t[~keep] = pad_value
    return t


def _note(family, ratio):
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), ratio)


def wgrad_family(ctx, srcs, Cout, Ho, Wo, K, S, pad, pm):
    """The family c2s_wgrad_path reports for the launch engine._wgrad_launch makes of these arguments, under the switches as
    they stand.  `ctx` needs its CU count only, `srcs` their shapes: no device is touched."""
    E, _ = _engine()
    fam = ctypes.c_int(-1)
    rc = E.lib().c2s_wgrad_path(ctypes.byref(E._wgrad_desc(ctx, srcs, Cout, Ho, Wo, K, S, pad, pm)), ctypes.byref(fam))
    assert rc == 0, E.lib().c2s_last_error()
    return fam.value


def _check_wgrad(name, ctx, srcs, Cout, Ho, Wo, K, S, pad, pm, observed, expected):
    """The reported family is the literal one, and its class is the one observed."""
    fam = wgrad_family(ctx, srcs, Cout, Ho, Wo, K, S, pad, pm)
    assert WGRAD_CLASS[fam] == observed, f"{name}: c2s_wgrad_path reports family {fam}, the weight gradient ran on {observed}"
    assert fam == expected, f"{name}: weight gradient on family {fam}, the table says {expected}"
    return fam


def _observed_wgrad(ctx, srcs, gout, Cout, Ho, Wo, K, S, pad, pm, so, sc, taps, valid, got):
    """The weight-gradient algorithm that produced `got`, observed, to hold against the library's report (_check_wgrad).  The
    split-K kernels and their fixed-order slice sum are deterministic and the algorithms round differently: `got` is
    bit-identical to the forced run of the algorithm that ran, and to that one only (c2s_wgrad_algorithms, reset to -1 in
    finally)."""
    E, _ = _engine()
    runs = {}
    try:
        for on in (0, 1):
            E.lib().c2s_wgrad_algorithms(on, on)
            runs[on] = torch.empty_like(got)
            E._wgrad_launch(ctx, srcs, gout, Cout, Ho, Wo, K, S, pad, pm, runs[on], so, sc, taps, 0, valid)
        torch.cuda.synchronize()
    finally:
        E.lib().c2s_wgrad_algorithms(-1, -1)
    if torch.equal(got, runs[0]):
        return "wgrad_direct"          # (also where the Winograd algorithm does not apply: both forced runs are direct)
    assert torch.equal(got, runs[1]), "the weight gradient is bit-identical to neither algorithm's forced run"
    return {3: "wgrad_f23", 4: "wgrad_f22"}[K]


def _fwd_kernel(ctx):
    pk, rec = ctx._packed, ctx.ws.pack_record
    if ("w", "fwd", "wino") in pk:
        return "wino16" if rec[("w", "fwd", "wino")][7] == 2 else "wino4"
    if ("w", "fwd", "s2w") in pk:
        return "s2wino"
    assert ("w", "fwd") in pk
    return "igemm"


def _dgrad_kernel(ctx, si):
    pk, rec = ctx._packed, ctx.ws.pack_record
    if ("w", "dgrad", "wino", si) in pk:
        return "wino16" if rec[("w", "dgrad", "wino", si)][7] == 2 else "wino4"
    if ("w", "dgrad", "s2d", si) in pk:
        return "s2dgrad"
    if ("w", "dgrad", si, 0) in pk and ("w", "dgrad", si, 1) in pk:
        return "xpair"
    assert ("w", "dgrad", si) in pk
    return "igemm"


# =================================================================================================
# conv2d: forward + data gradient (+ weight gradient) of one layer
# =================================================================================================
class Row(NamedTuple):
    id: str
    N: int
    chans: Tuple[int, ...]
    Cout: int
    H: int
    W: int
    K: int
    S: int
    mode: str
    acc: Tuple[int, ...]          # per source: prior gradient on the tape
    fwd: str                      # forward kernel it must reach
    dgrad: Tuple[str, ...]        # data-gradient kernel per source
    wgrad: int                    # weight-gradient family (c2s_wgrad_path)


ROWS = [
    # 8-wave Winograd (conv_winograd16.hip) forward + data gradient with the reflect adjoint
    Row("wino16", 3, (64,), 64, 64, 64, 3, 1, "reflect", (0,), "wino16", ("wino16",), 5),
    Row("wino16-acc", 3, (64,), 64, 64, 64, 3, 1, "reflect", (1,), "wino16", ("wino16",), 5),
    Row("wino16-5frames-acc", 5, (64,), 64, 32, 64, 3, 1, "reflect", (1,), "wino16", ("wino16",), 5),
    # ragged: partial tiles both ways; the data gradient into 32 channels runs on the implicit GEMM
    Row("wino16-ragged", 3, (32,), 72, 12, 40, 3, 1, "reflect", (0,), "wino16", ("igemm",), 0),
    Row("wino16-ragged-acc", 3, (32,), 72, 12, 40, 3, 1, "reflect", (1,), "wino16", ("igemm",), 0),
    # ... and the 8-wave data gradient into 72 channels (a half-empty second block of 64) on partial tiles
    Row("wino16-ragged-dgrad-acc", 3, (72,), 64, 12, 40, 3, 1, "reflect", (1,), "wino16", ("wino16",), 0),
    # 4-wave Winograd (conv_winograd.hip): 16 x 16 planes, ragged channel counts
    Row("wino4", 3, (128,), 128, 16, 16, 3, 1, "reflect", (0,), "wino4", ("wino4",), 2),
    Row("wino4-acc", 3, (128,), 128, 16, 16, 3, 1, "reflect", (1,), "wino4", ("wino4",), 2),
    Row("wino4-ragged-acc", 3, (36,), 64, 16, 32, 3, 1, "reflect", (1,), "wino4", ("igemm",), 5),
    Row("wino4-ragged-dgrad-acc", 3, (64,), 36, 16, 32, 3, 1, "reflect", (1,), "igemm", ("wino4",), 5),
    # two sources [up, skip] (UpConvBlock conv1), the prior on the second source only
    Row("two-sources-acc-skip", 3, (32, 64), 64, 32, 64, 3, 1, "reflect", (0, 1), "wino16", ("igemm", "wino16"), 4),
    # implicit GEMM 3x3 (conv_igemm.hip): Cout < 64, 4 x 4 maps, 32-channel decoder layers
    Row("igemm-cout32", 3, (64,), 32, 32, 32, 3, 1, "reflect", (0,), "igemm", ("wino16",), 5),
    Row("igemm-cout32-acc", 3, (64,), 32, 32, 32, 3, 1, "reflect", (1,), "igemm", ("wino16",), 5),
    Row("igemm-32ch", 3, (32,), 32, 32, 32, 3, 1, "reflect", (0,), "igemm", ("igemm",), 4),
    Row("igemm-32ch-acc", 3, (32,), 32, 32, 32, 3, 1, "reflect", (1,), "igemm", ("igemm",), 4),
    Row("igemm-4x4", 3, (128,), 128, 4, 4, 3, 1, "reflect", (0,), "igemm", ("igemm",), 0),
    Row("igemm-4x4-acc", 3, (128,), 128, 4, 4, 3, 1, "reflect", (1,), "igemm", ("igemm",), 0),
    # implicit GEMM 1x1
    Row("igemm-1x1-acc", 3, (64,), 32, 32, 32, 1, 1, "zeros", (1,), "igemm", ("igemm",), 1),
    # 4x4 stride 2: F(2x2,2x2) forward (conv_s2wino.hip) + data gradient (conv_s2dgrad.hip)
    Row("s2", 3, (64,), 64, 128, 128, 4, 2, "reflect", (0,), "s2wino", ("s2dgrad",), 6),
    Row("s2-acc", 3, (64,), 64, 128, 128, 4, 2, "reflect", (1,), "s2wino", ("s2dgrad",), 6),
    Row("s2-ragged", 3, (8,), 72, 24, 80, 4, 2, "reflect", (0,), "s2wino", ("s2dgrad",), 0),
    Row("s2-ragged-acc", 3, (8,), 72, 24, 80, 4, 2, "reflect", (1,), "s2wino", ("s2dgrad",), 0),
    # gy narrower than 32: implicit GEMM forward, transposed-row fallback of the data gradient (conv_xpair.hip)
    Row("xpair", 3, (64,), 64, 32, 32, 4, 2, "reflect", (0,), "igemm", ("xpair",), 2),
    Row("xpair-acc", 3, (64,), 64, 32, 32, 4, 2, "reflect", (1,), "igemm", ("xpair",), 2),
    # the XCD-aware (frame, tile) order of conv_igemm / conv_xpair in effect: 8 frames of 16 x 16 and 32 output channels, so
    # gridDim.y = 1 and the workgroups are a multiple of 8 at every split; the padded frames 1 and 3 return early after the remap
    Row("igemm-8frames-acc", 8, (32,), 32, 16, 16, 3, 1, "reflect", (1,), "igemm", ("igemm",), 2),
    Row("xpair-8frames-acc", 8, (32,), 32, 32, 32, 4, 2, "reflect", (1,), "igemm", ("xpair",), 2),
]


def _run_row(row: Row):
    E, L = _engine()
    g = _gen(row.id)
    N, K, S = row.N, row.K, row.S
    pad = 0 if K == 1 else 1
    pm = L.PAD_REFLECT if row.mode == "reflect" else L.PAD_ZEROS
    radj = int(row.mode == "reflect" and pad > 0)
    Cin = sum(row.chans)
    keep = _keep(N)
    Ho, Wo = (row.H + 2 * pad - K) // S + 1, (row.W + 2 * pad - K) // S + 1
    x = _randn((N, Cin, row.H, row.W), g, keep)
    w = torch.randn(row.Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
    b = torch.randn(row.Cout, generator=g)
    gout = _randn((N, row.Cout, Ho, Wo), g, keep)
    prior = torch.zeros_like(x)
    sentinel = torch.zeros(x.shape, dtype=torch.bool)
    ctx = _ctx({"w": w, "b": b})
    srcs, lo = [], 0
    for si, c in enumerate(row.chans):
        srcs.append(x[:, lo:lo + c].contiguous().cuda())
        if row.acc[si]:
            p = _randn((N, c, row.H, row.W), g, keep, SENTINEL)
            prior[:, lo:lo + c] = p
            sentinel[~keep, lo:lo + c] = True
            ctx.tape.grads[srcs[-1].data_ptr()] = p.cuda()
        lo += c
    vd, gd = keep.int().cuda(), gout.cuda()
    out = E.conv2d(ctx, srcs, "w", "b", K, S, pad, pm, vd)
    ctx.tape.grads[out.data_ptr()] = gd
    ctx.tape.backward()
    torch.cuda.synchronize()
    fwd = _fwd_kernel(ctx)
    dgrad = tuple(_dgrad_kernel(ctx, si) for si in range(len(srcs)))
    wk = _observed_wgrad(ctx, srcs, gd, row.Cout, Ho, Wo, K, S, pad, pm, Cin * K * K, K * K, list(range(K * K)), vd,
                         ctx.g["w"])
    assert (fwd, dgrad) == (row.fwd, row.dgrad), f"{row.id}: reached {fwd} / {dgrad}, the table says {row.fwd} / {row.dgrad}"
    REACHED_WGRAD[row.id] = {_check_wgrad(row.id, ctx, srcs, row.Cout, Ho, Wo, K, S, pad, pm, wk, row.wgrad)}
    REACHED[row.id] = {(k, a, radj) for k, a in zip(dgrad, row.acc)} | {(wk, 0, 0)}

    got_gx = torch.cat([ctx.tape.grads[s.data_ptr()].cpu() for s in srcs], 1)
    cd = torch.cat([torch.full((1, c, 1, 1), float(C_FAMILY[k])) for k, c in zip(dgrad, row.chans)], 1)
    c = {"fwd": C_FAMILY[fwd], "dgrad": cd, "wgrad": C_FAMILY[wk]}
    ratios = R.check_conv(out.cpu(), got_gx, ctx.g["w"].cpu(), x, w, b, gout, keep, S, pad, row.mode, c, prior=prior,
                          sentinel=sentinel)
    # the same ratios per source (kernel family) for the record
    ref = R.conv_refs(x[keep], w, b, gout[keep], S, pad, row.mode)
    lo = 0
    for k, cs in zip(dgrad, row.chans):
        sl = slice(lo, lo + cs)
        p = prior[keep][:, sl].double()
        _note(k, R.bound_ratio(got_gx[keep][:, sl], ref["gx"][:, sl] + p, ref["Agx"][:, sl] + p.abs()))
        lo += cs
    _note(fwd, ratios["fwd"])
    _note(wk, ratios["wgrad"])
    print(f"\n{row.id}: fwd {fwd} {ratios['fwd']:.2f}  dgrad {'/'.join(dgrad)} {ratios['dgrad']:.2f}  {wk} {ratios['wgrad']:.2f}")


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_conv2d_path(row):
    _run_row(row)


# =================================================================================================
# transposed and depthwise convolutions: the "existing gradient" branch
# =================================================================================================
TRANSPOSE_SHAPES = [(2, 128, 64, 4, 4), (2, 64, 32, 16, 16), (1, 32, 32, 64, 64)]     # no frame flags on this op
TRANSPOSE_WGRAD = {TRANSPOSE_SHAPES[0]: 0, TRANSPOSE_SHAPES[1]: 2, TRANSPOSE_SHAPES[2]: 6}     # weight-gradient family


def _run_transpose(shape):
    E, L = _engine()
    N, Cin, Cout, H, W = shape
    g = _gen(f"transpose{shape}")
    keep = torch.ones(N, dtype=torch.bool)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, 4, 4, generator=g) / math.sqrt(Cin * 4)
    b = torch.randn(Cout, generator=g)
    gout = torch.randn(N, Cout, 2 * H, 2 * W, generator=g)
    prior = torch.randn(x.shape, generator=g)
    ctx = _ctx({"w": w, "b": b})
    xd = x.cuda()
    ctx.tape.grads[xd.data_ptr()] = prior.cuda()
    out = E.conv_transpose2d(ctx, xd, "w", "b")
    gd = gout.cuda()
    ctx.tape.grads[out.data_ptr()] = gd
    ctx.tape.backward()
    torch.cuda.synchronize()
    assert ("w", "dgrad") in ctx._packed and ("w", "fwd", 0) in ctx._packed
    # dW = conv4x4s2 weight gradient with (input = gout, gout = x), as engine.conv_transpose2d launches it
    wk = _observed_wgrad(ctx, [gd], xd, Cin, H, W, 4, 2, 1, L.PAD_ZEROS, Cout * 16, 16, list(range(16)), None, ctx.g["w"])
    REACHED_WGRAD[f"transpose{shape}"] = {_check_wgrad(f"transpose{shape}", ctx, [gd], Cin, H, W, 4, 2, 1, L.PAD_ZEROS, wk,
                                                       TRANSPOSE_WGRAD[shape])}
    REACHED[f"transpose{shape}"] = {("igemm", 1, 0), (wk, 0, 0)}
    c = {"fwd": C_FAMILY["xpair"], "dgrad": C_FAMILY["igemm"], "wgrad": C_FAMILY[wk]}
    ratios = R.check_conv(out.cpu(), ctx.tape.grads[xd.data_ptr()].cpu(), ctx.g["w"].cpu(), x, w, b, gout, keep, 2, 1,
                          "zeros", c, prior=prior, transpose=True)
    _note("xpair", ratios["fwd"])
    _note("igemm", ratios["dgrad"])
    _note(wk, ratios["wgrad"])
    print(f"\ntranspose{shape}: {ratios}")


@pytest.mark.parametrize("shape", TRANSPOSE_SHAPES)
def test_conv_transpose_accumulate(shape):
    _run_transpose(shape)


DEPTHWISE = [(K, S, hw) for K, S in [(3, 1), (4, 2)] for hw in (16, 40, 6)]     # 40: float4 spans; 6: one output per thread


def _run_depthwise(K, S, hw):
    E, L = _engine()
    N, Cc = 3, 64
    Hin, Win = hw, hw + (8 if hw == 40 else 0)
    g = _gen(f"dw{K}{S}{hw}")
    keep = _keep(N)
    Ho, Wo = (Hin + 2 - K) // S + 1, (Win + 2 - K) // S + 1
    x = _randn((N, Cc, Hin, Win), g, keep)
    w = torch.randn(Cc, 1, K, K, generator=g)
    gout = _randn((N, Cc, Ho, Wo), g, keep)
    prior = _randn(x.shape, g, keep, SENTINEL)
    sentinel = (~keep).view(N, 1, 1, 1).expand(x.shape).clone()
    ctx = _ctx({"w": w})
    xd = x.cuda()
    ctx.tape.grads[xd.data_ptr()] = prior.cuda()
    out = E.depthwise_conv2d(ctx, xd, "w", K, S, 1, L.PAD_REFLECT, keep.int().cuda())
    ctx.tape.grads[out.data_ptr()] = gout.cuda()
    ctx.tape.backward()
    torch.cuda.synchronize()
    # one kernel each (c2s_dwconv_dgrad / c2s_dwconv_wgrad, no alternative algorithm): nothing to observe, fixed entries
    REACHED[f"dw{K}{S}{hw}"] = {("dw", 1, 1), ("dw_wgrad", 0, 0)}
    c = {"fwd": C_FAMILY["dw"], "dgrad": C_FAMILY["dw"], "wgrad": C_FAMILY["dw_wgrad"]}
    ratios = R.check_conv(out.cpu(), ctx.tape.grads[xd.data_ptr()].cpu(), ctx.g["w"].cpu(), x, w, None, gout, keep, S, 1,
                          "reflect", c, prior=prior, sentinel=sentinel, groups=Cc)
    _note("dw", max(ratios["fwd"], ratios["dgrad"]))
    _note("dw_wgrad", ratios["wgrad"])
    print(f"\ndw{K}{S}{hw}: {ratios}")


@pytest.mark.parametrize("K,S,hw", DEPTHWISE)
def test_depthwise_accumulate(K, S, hw):
    _run_depthwise(K, S, hw)


# =================================================================================================
# weight gradients: one weight written twice in a tape (grad_sink accumulate = 1)
# =================================================================================================
WGRAD_TWICE = [
    # (K, S, N, C, Cout, H, W): both algorithms of the layer, forced through c2s_wgrad_algorithms
    (3, 1, 3, 64, 64, 32, 32),          # F(2x2,3x3) and direct
    (4, 2, 3, 64, 64, 64, 64),          # F(2x2,2x2) and direct
]
WGRAD_TWICE_FAMILY = {(3, 1): {True: 5, False: 1}, (4, 2): {True: 6, False: 1}}      # (K, S) -> forced fast / forced direct


def _two_layer_refs(x1, x2, w, gout1, gout2, keep, K, S, pad):
    r1 = R.conv_refs(x1[keep], w, None, gout1[keep], S, pad, "reflect")
    r2 = R.conv_refs(x2[keep], w, None, gout2[keep], S, pad, "reflect")
    return r1["gw"] + r2["gw"], r1["Agw"] + r2["Agw"]


def _wgrad_twice(K, S, N, Cc, Cout, H, W, fast):
    E, L = _engine()
    g = _gen(f"twice{K}{S}")
    pad = 1
    keep = _keep(N)
    Ho, Wo = (H + 2 - K) // S + 1, (W + 2 - K) // S + 1
    x1, x2 = _randn((N, Cc, H, W), g, keep), _randn((N, Cc, H, W), g, keep)
    w = torch.randn(Cout, Cc, K, K, generator=g) / math.sqrt(Cc * K * K)
    g1, g2 = _randn((N, Cout, Ho, Wo), g, keep), _randn((N, Cout, Ho, Wo), g, keep)
    ctx = _ctx({"w": w})
    try:
        E.lib().c2s_wgrad_algorithms(int(fast) if K == 3 else -1, int(fast) if K == 4 else -1)
        v = keep.int().cuda()
        x1d = x1.cuda()
        fam = wgrad_family(ctx, [x1d], Cout, Ho, Wo, K, S, pad, L.PAD_REFLECT)
        y1 = E.conv2d(ctx, [x1d], "w", None, K, S, pad, L.PAD_REFLECT, v, need_input_grad=False)
        y2 = E.conv2d(ctx, [x2.cuda()], "w", None, K, S, pad, L.PAD_REFLECT, v, need_input_grad=False)
        ctx.tape.grads[y1.data_ptr()] = g1.cuda()
        ctx.tape.grads[y2.data_ptr()] = g2.cuda()
        ctx.tape.backward()
        torch.cuda.synchronize()
    finally:
        E.lib().c2s_wgrad_algorithms(-1, -1)
    assert fam == WGRAD_TWICE_FAMILY[K, S][fast], f"forced {'fast' if fast else 'direct'}: weight gradient on family {fam}"
    wk = WGRAD_CLASS[fam]
    assert (wk != "wgrad_direct") == fast
    ref, A = _two_layer_refs(x1, x2, w, g1, g2, keep, K, S, pad)
    ratio = R.assert_within(f"weight gradient written twice ({wk})", ctx.g["w"], ref, A, C_FAMILY[wk], R.FROB_GRAD)
    _note(wk, ratio)
    print(f"\nwgrad twice {wk}: {ratio:.2f}")
    return wk, fam, ctx.g["w"].cpu()


@pytest.mark.parametrize("K,S,N,Cc,Cout,H,W", WGRAD_TWICE)
def test_weight_gradient_written_twice(K, S, N, Cc, Cout, H, W):
    wk_fast, fam_fast, fast = _wgrad_twice(K, S, N, Cc, Cout, H, W, True)
    wk_direct, fam_direct, direct = _wgrad_twice(K, S, N, Cc, Cout, H, W, False)
    assert not torch.equal(fast, direct), "the forced weight-gradient algorithms must be different kernels"
    REACHED_WGRAD[f"twice{K}{S}"] = {fam_fast, fam_direct}
    REACHED[f"twice{K}{S}"] = {(wk_fast, 0, 0), (wk_fast, 1, 0), (wk_direct, 0, 0), (wk_direct, 1, 0)}


def test_reduce_batch_mixed_accumulating_and_fresh(monkeypatch):
    """C2S_REDUCE_BATCH: the batched slice sums hold the first write of every weight; a weight written a second time in
    the tape (w2) must add its sum after the batch, next to a layer written once (w1).  Two steps on one workspace (job
    table built, then reused); bit-identical to the per-layer sums and within the bound of the float64 chain."""
    E, L = _engine()
    g = _gen("reduce-batch")
    N, Cc, H, W = 3, 64, 32, 32
    keep = _keep(N)
    x = _randn((N, Cc, H, W), g, keep)
    w1 = torch.randn(Cc, Cc, 3, 3, generator=g) / 24
    w2 = torch.randn(Cc, Cc, 3, 3, generator=g) / 24
    ga, gb = _randn((N, Cc, H, W), g, keep), _randn((N, Cc, H, W), g, keep)
    v = keep.int().cuda()
    results, acc_slab = {}, None
    for batched in (False, True):
        monkeypatch.setattr(E, "REDUCE_BATCH", batched)
        ctx0 = _ctx({"w1": w1, "w2": w2})
        for _ in range(2):
            ctx = E.Ctx(ctx0.p, ctx0.b, ctx0.g, ctx0.ws, True, E.Tape())
            xd = x.cuda()
            h = E.conv2d(ctx, [xd], "w1", None, 3, 1, 1, L.PAD_REFLECT, v, need_input_grad=False)
            ya = E.conv2d(ctx, [xd], "w2", None, 3, 1, 1, L.PAD_REFLECT, v, need_input_grad=False)
            yb = E.conv2d(ctx, [h], "w2", None, 3, 1, 1, L.PAD_REFLECT, v)
            ctx.tape.grads[ya.data_ptr()] = ga.cuda()
            ctx.tape.grads[yb.data_ptr()] = gb.cuda()
            ctx.tape.backward()
            torch.cuda.synchronize()
            if batched:
                assert ctx.ws.reduce_plan is not None and ctx.ws.reduce_plan["njobs"] == 2
                assert not ctx.ws.reduce_jobs and not ctx.ws.reduce_post
                # w2's accumulating slab buffer survives the plan (re)build and is reused by the next step
                slabs = [b for k, b in ctx.ws.bufs.items() if k.startswith("wgrad_slabs:") and k.endswith(":acc0")]
                assert len(slabs) == 1, "the accumulating slab buffer was dropped from the workspace"
                assert acc_slab is None or slabs[0].data_ptr() == acc_slab
                acc_slab = slabs[0].data_ptr()
        results[batched] = (ctx.g["w1"].cpu(), ctx.g["w2"].cpu())
    # no entries: the kernels are the default ones of the table; the weight-gradient accumulate paths are observed by
    # test_weight_gradient_written_twice
    REACHED["reduce-batch"] = set()
    # float64 chain (and the same chain on absolute values for the bound)
    def chain(xs, a1, a2, gas, gbs):
        xs = xs[keep].double()
        a1 = a1.double().requires_grad_(True)
        a2 = a2.double().requires_grad_(True)
        pad = lambda t: torch.nn.functional.pad(t, (1, 1, 1, 1), mode="reflect")
        hh = torch.nn.functional.conv2d(pad(xs), a1)
        ya_ = torch.nn.functional.conv2d(pad(xs), a2)
        yb_ = torch.nn.functional.conv2d(pad(hh), a2)
        torch.autograd.backward([ya_, yb_], [gas[keep].double(), gbs[keep].double()])
        return a1.grad, a2.grad
    r1, r2 = chain(x, w1, w2, ga, gb)
    A1, A2 = chain(x.abs(), w1.abs(), w2.abs(), ga.abs(), gb.abs())
    c = C_FAMILY["wgrad_f23"] + C_FAMILY["wino16"]      # w1's gradient also carries the rounding of h and of its gradient
    for batched in (False, True):
        q1 = R.assert_within(f"w1 (batched {batched})", results[batched][0], r1, A1, c, R.FROB_GRAD)
        q2 = R.assert_within(f"w2 written twice (batched {batched})", results[batched][1], r2, A2, c, R.FROB_GRAD)
        print(f"\nreduce batch {batched}: w1 {q1:.2f}  w2 {q2:.2f}")
    assert torch.equal(results[True][0], results[False][0]) and torch.equal(results[True][1], results[False][1])


# =================================================================================================
# coverage: the paths the table reached
# =================================================================================================
EXPECTED = {
    ("wino16", 0, 1), ("wino16", 1, 1), ("wino4", 0, 1), ("wino4", 1, 1),
    ("igemm", 0, 1), ("igemm", 1, 1), ("igemm", 1, 0),
    ("s2dgrad", 0, 1), ("s2dgrad", 1, 1), ("xpair", 0, 1), ("xpair", 1, 1),
    ("dw", 1, 1),
    ("wgrad_direct", 0, 0), ("wgrad_direct", 1, 0), ("wgrad_f23", 0, 0), ("wgrad_f23", 1, 0),
    ("wgrad_f22", 0, 0), ("wgrad_f22", 1, 0), ("dw_wgrad", 0, 0),
}
EXPECTED_WGRAD = {0, 1, 2, 4, 5, 6}      # (3, the first-layer form, is reached by test_conv_modes_gpu.py: seven in all)


def test_reached_paths_are_the_table(monkeypatch):
    """Every (kernel, accumulate, reflect_adjoint) and every weight-gradient family the table reached, against the expected
    sets: a dispatch change that moves a row to another kernel fails its row, one that drops a path altogether fails here.
    Rows not run yet in this session (-k selections) run here."""
    for row in ROWS:
        if row.id not in REACHED:
            _run_row(row)
    for shape in TRANSPOSE_SHAPES:
        if f"transpose{shape}" not in REACHED:
            _run_transpose(shape)
    for K, S, hw in DEPTHWISE:
        if f"dw{K}{S}{hw}" not in REACHED:
            _run_depthwise(K, S, hw)
    for case in WGRAD_TWICE:
        if f"twice{case[0]}{case[1]}" not in REACHED:
            test_weight_gradient_written_twice(*case)
    if "reduce-batch" not in REACHED:
        test_reduce_batch_mixed_accumulating_and_fresh(monkeypatch)
    reached = set().union(*REACHED.values())
    print("\nworst |err| / (u * A) per kernel family: " + "  ".join(f"{k} {v:.2f}" for k, v in sorted(OBSERVED.items())))
    assert reached == EXPECTED, f"missing {sorted(EXPECTED - reached)}, unexpected {sorted(reached - EXPECTED)}"
    families = set().union(*REACHED_WGRAD.values())
    assert families == EXPECTED_WGRAD, f"weight-gradient families reached: {sorted(families)}, expected {sorted(EXPECTED_WGRAD)}"
