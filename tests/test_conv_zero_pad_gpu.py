"""The 3x3 stride-1 convolution kernels under ZERO padding against the float64 references of tests/conv_ref.py, element by
element: the 8-wave and 4-wave Winograd kernels, the implicit GEMM (split and unsplit tiles), the split-precision bf16x3
kernel and the data gradient behind the first-layer kernel.

Under zero padding these kernels take other code than under reflect padding: the data gradient runs with
reflect_adjoint = 0 (no fold in tile_store, in the Winograd raw-patch transforms or in the bf16x3 border rules), staging takes
the `ok = inside` branch of tile_pixel_offset and the Winograd kernels' own equivalents, and the F(2x3,3x3) weight gradient
reads a zero halo.  A fault that writes a mirrored value where a zero belongs touches border rows and columns only; one that
keeps a stale accumulate when the adjoint is off touches the accumulating rows only.  Before this file those paths were held
by the whole-tensor Frobenius bars of test_ops_gpu.py alone (finite padded frames, an empty tape).

The conventions are those of test_conv_paths_gpu.py / test_conv_modes_gpu.py, and the helpers are theirs: every row has
mode = "zeros", K = 3, S = 1 and a bias; N = 3 with frame 1 padded (valid = 0), NaN in x and gout; an accumulating row seeds
the tape with a prior gradient that carries the sentinel 1234.5 on the padded frame, bit-identical afterwards; the weight
gradient must be finite.  The launches are observed with the spy of test_conv_modes_gpu around engine._run_conv: every row
asserts its set of (family, op, accumulate, reflect_adjoint) with reflect_adjoint == 0 throughout, and
test_reached_paths_are_the_table the whole set.  The weight-gradient family c2s_wgrad_path reports is held against the row's
literal and its class against the forced runs (_observed_wgrad).  Rows of the implicit GEMM also state the tile split
(c2s_conv_igemm_split, or the forced one): the small rows take the split tiles of test_conv_split_gpu.py by the rule, two rows
force 1 and 2.

Bars, unchanged from those files: |got - ref64| <= c * 2^-24 * A element by element with c = C_FAMILY[family] (wino16 12,
wino4 10, igemm and smallcin 20, wgrad_direct 12, wgrad_f23 4), (2^-16 + 20 * 2^-24) * A for bf16x3, and the Frobenius bars
2e-6 / 5e-6 (5e-5 for bf16x3 results).

Observed worst ratios max |err| / (u * A) over the zero-padded rows on an MI355X (printed with -s; u = 2^-24, bf16x3 2^-16):

    wino16 3.14   wino4 2.77   igemm 5.60   smallcin 3.93   bf16x3 0.11   wgrad_direct 2.64   wgrad_f23 0.95

No row exceeds its family's constant; the ratios sit where the reflect rows of the two older files do (wino16 2.68, wino4 2.17,
igemm 5.13, smallcin 5.51, bf16x3 0.13, wgrad_direct 3.11, wgrad_f23 1.43).

Found by these rows' whole-model companion (test_models_ctor_gpu.py): c2s_conv_igemm refused two sources whose first has 24
or 40 channels ("C0 must be a multiple of 16"), though its K loop only needs whole chunks (4 channels for 3x3); the two
z-igemm-two-sources-24-40 / 12-20 rows hold the relaxed check to float64.

The rows can fail: with c2s_conv3x3_winograd16 launching its reflect-adjoint kernel whenever `accumulate` is set (a local
build, not part of the project; it changes values only: a zero-padded accumulating data gradient gets the fold of the
mirrored border rows and columns), z-wino16-acc, z-wino16-ragged-dgrad-acc and z-two-sources-acc-skip fail here (data
gradient Frobenius error 0.10 - 0.15) and so does the train step of zeros-utae-64 in test_models_ctor_gpu.py, while the 552
tests of test_ops_gpu.py, test_conv_paths_gpu.py, test_conv_modes_gpu.py, test_conv_rect_gpu.py,
test_strided_geometry_gpu.py, test_conv_split_gpu.py, test_models_gpu.py, test_models_rect_gpu.py, test_configs_gpu.py and
test_frozen_gpu.py all pass under that build.
"""
import ctypes
import math
from typing import NamedTuple, Optional, Tuple

import pytest
import torch

import conv_ref as R
from test_conv_modes_gpu import BOUNDS as MODE_BOUNDS
from test_conv_modes_gpu import _spy
from test_conv_paths_gpu import C_FAMILY, SENTINEL, _check_wgrad, _ctx, _gen, _keep, _observed_wgrad, _randn

pytestmark = pytest.mark.gpu

# family -> (c in units of 2^-24, Frobenius bar forward, Frobenius bar gradient, u of the printed ratio)
BOUNDS = dict(MODE_BOUNDS)
BOUNDS["wino16"] = (C_FAMILY["wino16"], R.FROB_FWD, R.FROB_GRAD, R.U)
BOUNDS["wino4"] = (C_FAMILY["wino4"], R.FROB_FWD, R.FROB_GRAD, R.U)
OBSERVED = {}           # family -> worst max |err| / (u * A), u of the family
REACHED = {}            # row id -> set of (family, op, accumulate, reflect_adjoint)
REACHED_WGRAD = {}      # row id -> set of weight-gradient families (c2s_wgrad_path)
REACHED_SPLIT = {}      # row id -> set of tile splits of its implicit-GEMM launches


class ZRow(NamedTuple):
    id: str
    conv_mode: str                # engine.CONV_MODE while the row runs
    wino16: bool                  # engine.WINO16 while the row runs
    chans: Tuple[int, ...]
    Cout: int
    H: int
    W: int
    acc: Tuple[int, ...]          # per source: prior gradient on the tape
    fwd: str                      # forward family it must reach
    dgrad: Tuple[str, ...]        # data-gradient family per source
    wgrad: int                    # weight-gradient family (c2s_wgrad_path)
    split: Optional[int] = None   # C2S_IGEMM_SPLIT forced while the row runs (None: the rule)


F32, BX = "f32", "bf16x3"
ROWS = [
    # 8-wave Winograd (conv_winograd16.hip): forward and data gradient without the adjoint
    ZRow("z-wino16", F32, True, (64,), 64, 64, 64, (0,), "wino16", ("wino16",), 5),
    ZRow("z-wino16-acc", F32, True, (64,), 64, 64, 64, (1,), "wino16", ("wino16",), 5),
    # partial tiles both ways; the data gradient into 32 channels runs on the implicit GEMM
    ZRow("z-wino16-ragged-acc", F32, True, (32,), 72, 12, 40, (1,), "wino16", ("igemm",), 0),
    # ... and the other direction: the 8-wave data gradient from 32 into 72 channels on partial tiles, forward on the GEMM
    ZRow("z-wino16-ragged-dgrad-acc", F32, True, (72,), 32, 12, 40, (1,), "igemm", ("wino16",), 0),
    # two sources [up, skip], the prior on the skip source
    ZRow("z-two-sources-acc-skip", F32, True, (32, 64), 64, 32, 64, (0, 1), "wino16", ("igemm", "wino16"), 4),
    # 4-wave Winograd (conv_winograd.hip): WINO16 off on the 64 x 64 shape; ragged channel counts both ways
    ZRow("z-wino4", F32, False, (64,), 64, 64, 64, (0,), "wino4", ("wino4",), 5),
    ZRow("z-wino4-acc", F32, False, (64,), 64, 64, 64, (1,), "wino4", ("wino4",), 5),
    ZRow("z-wino4-16x16-acc", F32, True, (128,), 128, 16, 16, (1,), "wino4", ("wino4",), 2),
    ZRow("z-wino4-ragged-acc", F32, True, (36,), 64, 16, 32, (1,), "wino4", ("igemm",), 5),
    ZRow("z-wino4-ragged-dgrad-acc", F32, True, (64,), 36, 16, 32, (1,), "igemm", ("wino4",), 5),
    # implicit GEMM (conv_igemm.hip): planes that are all border, ragged channels and planes, Cout = 15, two sources
    ZRow("z-igemm-4x4", F32, True, (64,), 64, 4, 4, (0,), "igemm", ("igemm",), 0),
    ZRow("z-igemm-4x4-acc", F32, True, (64,), 64, 4, 4, (1,), "igemm", ("igemm",), 0),
    ZRow("z-igemm-2x2-acc", F32, True, (64,), 64, 2, 2, (1,), "igemm", ("igemm",), 0),
    ZRow("z-igemm-24to40-acc", F32, True, (24,), 40, 24, 40, (1,), "igemm", ("igemm",), 0),
    ZRow("z-igemm-cout15-acc", F32, True, (32,), 15, 32, 32, (1,), "igemm", ("igemm",), 1),
    ZRow("z-igemm-two-sources-acc", F32, True, (16, 8), 32, 32, 32, (1, 1), "igemm", ("igemm", "igemm"), 1),
    # a first source of 24 and of 12 channels: whole chunks of 4 channels, no multiple of 16 (decoder widths 24 and 40 put
    # such an [up, skip] pair in front of UpConvBlock's conv1; c2s_conv_igemm used to refuse them)
    ZRow("z-igemm-two-sources-24-40-acc", F32, True, (24, 40), 24, 16, 16, (1, 1), "igemm", ("igemm", "igemm"), 2),
    ZRow("z-igemm-two-sources-12-20-acc", F32, True, (12, 20), 32, 8, 8, (0, 1), "igemm", ("igemm", "igemm"), 0),
    # the rule splits every row above on a device of 256 CUs (fewer than two workgroups per CU); the unsplit tile and split 2
    ZRow("z-igemm-24to40-split1-acc", F32, True, (24,), 40, 24, 40, (1,), "igemm", ("igemm",), 0, 1),
    ZRow("z-igemm-24to40-split2-acc", F32, True, (24,), 40, 24, 40, (1,), "igemm", ("igemm",), 0, 2),
    # split-precision kernel (conv_bf16x3.hip): no border rule at all
    ZRow("zb-acc", BX, True, (64,), 64, 64, 64, (1,), "bf16x3", ("bf16x3",), 5),
    ZRow("zb-4x4-acc", BX, True, (128,), 128, 4, 4, (1,), "bf16x3", ("bf16x3",), 0),
    ZRow("zb-2x2-acc", BX, True, (64,), 64, 2, 2, (1,), "bf16x3", ("bf16x3",), 0),
    # 3-pixel axes stay on the implicit GEMM in this mode (engine._family_3x3), whatever the padding
    ZRow("zb-3x5-acc", BX, True, (64,), 64, 3, 5, (1,), "igemm", ("igemm",), 0),
    ZRow("zb-5x3-acc", BX, True, (64,), 64, 5, 3, (1,), "igemm", ("igemm",), 0),
    # the first layer: the data gradient into an input that wants one (implicit GEMM), added to a prior
    ZRow("z-first-10-dgrad-acc", F32, True, (10,), 64, 32, 32, (1,), "smallcin", ("igemm",), 3),
]
N = 3


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _note(family, ratio24):
    """ratio24 = max |err| / (2^-24 * A); recorded in the u of the family."""
    ratio = ratio24 * R.U / BOUNDS[family][3] if family in BOUNDS else ratio24
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), ratio)
    return ratio


def _spy_splits(m, E, splits):
    """On top of the launch spy: the tile split of every implicit-GEMM launch, as c2s_conv_igemm takes it (the forced one,
    else the rule for this device)."""
    import os
    inner = E._run_conv

    def run_conv(ctx, plan, *args, **kw):
        if plan.family == "igemm":
            for launch in plan.launches:
                forced = os.environ.get("C2S_IGEMM_SPLIT")
                splits.add(int(forced) if forced else E.lib().c2s_conv_igemm_split(ctypes.byref(launch.desc), 0))
        return inner(ctx, plan, *args, **kw)

    m.setattr(E, "_run_conv", run_conv)


def _run_row(row: ZRow, monkeypatch):
    E, L = _engine()
    g = _gen(row.id)
    K, S, pad, pm = 3, 1, 1, L.PAD_ZEROS
    Cin, H, W = sum(row.chans), row.H, row.W
    keep = _keep(N)
    x = _randn((N, Cin, H, W), g, keep)
    w = torch.randn(row.Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
    b = torch.randn(row.Cout, generator=g)
    gout = _randn((N, row.Cout, H, W), g, keep)
    prior = torch.zeros_like(x)
    ctx = _ctx({"w": w, "b": b})
    srcs, lo = [], 0
    for si, c in enumerate(row.chans):
        srcs.append(x[:, lo:lo + c].contiguous().cuda())
        if row.acc[si]:
            p = _randn((N, c, H, W), g, keep, SENTINEL)
            prior[:, lo:lo + c] = p
            ctx.tape.grads[srcs[-1].data_ptr()] = p.cuda()
        lo += c
    vd, gd = keep.int().cuda(), gout.cuda()
    splits = set()
    with monkeypatch.context() as m:                # the switches and the spies end with the row
        m.setattr(E, "CONV_MODE", row.conv_mode)
        m.setattr(E, "WINO16", row.wino16)
        if row.split is None:
            m.delenv("C2S_IGEMM_SPLIT", raising=False)
        else:
            m.setenv("C2S_IGEMM_SPLIT", str(row.split))
        calls = _spy(m, E)
        _spy_splits(m, E, splits)
        out = E.conv2d(ctx, srcs, "w", "b", K, S, pad, pm, vd)
        ctx.tape.grads[out.data_ptr()] = gd
        ctx.tape.backward()
        torch.cuda.synchronize()
        wk = _observed_wgrad(ctx, srcs, gd, row.Cout, H, W, K, S, pad, pm, Cin * K * K, K * K, list(range(K * K)), vd,
                             ctx.g["w"])
    # the kernels that ran: no launch with the reflect adjoint
    fwd = [c for c in calls if c[1] == "fwd"]
    dgrad = sorted((c for c in calls if c[1] == "dgrad"), key=lambda c: c[2])
    assert len(calls) == len(fwd) + len(dgrad) and len(fwd) == 1, f"{row.id}: launches {calls}"
    assert fwd[0] == (row.fwd, "fwd", None, 0, 0), f"{row.id}: forward launch {fwd[0]}, the table says {row.fwd}"
    want = [(k, "dgrad", si, a, 0) for si, (k, a) in enumerate(zip(row.dgrad, row.acc))]
    assert dgrad == want, f"{row.id}: data-gradient launches {dgrad}, the table says {want}"
    if row.split is not None:
        assert splits == {row.split}, f"{row.id}: implicit-GEMM launches at splits {sorted(splits)}"
    REACHED_WGRAD[row.id] = {_check_wgrad(row.id, ctx, srcs, row.Cout, H, W, K, S, pad, pm, wk, row.wgrad)}
    REACHED[row.id] = {(c[0], c[1], c[3], c[4]) for c in calls} | {(wk, "wgrad", 0, 0)}
    REACHED_SPLIT[row.id] = splits

    # the values
    ref = R.conv_refs(x[keep], w, b, gout[keep], S, pad, "zeros")
    c, frob_fwd, _, _ = BOUNDS[row.fwd]
    shown = [f"fwd {row.fwd} {_note(row.fwd, R.assert_within('forward', out.cpu()[keep], ref['y'], ref['Ay'], c, frob_fwd)):.2f}"]
    lo = 0
    for si, (k, cs) in enumerate(zip(row.dgrad, row.chans)):
        sl = slice(lo, lo + cs)
        got = ctx.tape.grads[srcs[si].data_ptr()].cpu()
        p = prior[keep][:, sl].double()
        c, _, frob_grad, _ = BOUNDS[k]
        q = R.assert_within(f"data gradient of source {si}", got[keep], ref["gx"][:, sl] + p, ref["Agx"][:, sl] + p.abs(), c,
                            frob_grad)
        shown.append(f"dgrad[{si}] {k} {_note(k, q):.2f}")
        if row.acc[si]:
            same = got[~keep].view(torch.int32) == prior[~keep][:, sl].view(torch.int32)
            assert bool((prior[~keep][:, sl] == SENTINEL).all()) and bool(same.all()), \
                f"{row.id}: padded-frame gradient of source {si} overwritten: {int((~same).sum())} elements"
        lo += cs
    gw = ctx.g["w"].cpu()
    assert bool(torch.isfinite(gw).all()), f"{row.id}: weight gradient not finite (a kernel read a padded frame?)"
    q = R.assert_within("weight gradient", gw, ref["gw"], ref["Agw"], C_FAMILY[wk], R.FROB_GRAD)
    _note(wk, q)
    print(f"\n{row.id}: " + "  ".join(shown) + f"  {wk} {q:.2f}  igemm splits {sorted(splits)}")


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_zero_padded_3x3(row, monkeypatch):
    _run_row(row, monkeypatch)


# =================================================================================================
# coverage: the paths the table reached
# =================================================================================================
EXPECTED = {
    ("wino16", "fwd", 0, 0), ("wino4", "fwd", 0, 0), ("igemm", "fwd", 0, 0), ("bf16x3", "fwd", 0, 0), ("smallcin", "fwd", 0, 0),
    ("wino16", "dgrad", 0, 0), ("wino16", "dgrad", 1, 0), ("wino4", "dgrad", 0, 0), ("wino4", "dgrad", 1, 0),
    ("igemm", "dgrad", 0, 0), ("igemm", "dgrad", 1, 0), ("bf16x3", "dgrad", 1, 0),
    ("wgrad_direct", "wgrad", 0, 0), ("wgrad_f23", "wgrad", 0, 0),
}
EXPECTED_WGRAD = {0, 1, 2, 3, 4, 5}      # both F(2x3,3x3) forms (4, 5) and the direct ones (0 generic, 1 / 2 tiles, 3 first layer)


def test_reached_paths_are_the_table(monkeypatch):
    """Every (family, op, accumulate, reflect_adjoint) and every weight-gradient family the table reached, against the
    expected sets: a dispatch change that moves a row to another kernel fails its row, one that drops a path altogether fails
    here.  Rows not run yet in this session (-k selections) run here."""
    for row in ROWS:
        if row.id not in REACHED:
            _run_row(row, monkeypatch)
    reached = set().union(*REACHED.values())
    print("\nworst |err| / (u * A) per kernel family: " + "  ".join(f"{k} {v:.2f}" for k, v in sorted(OBSERVED.items())))
    assert all(r[3] == 0 for r in reached), "a zero-padded row launched with the reflect adjoint"
    assert reached == EXPECTED, f"missing {sorted(EXPECTED - reached)}, unexpected {sorted(reached - EXPECTED)}"
    families = set().union(*REACHED_WGRAD.values())
    assert families == EXPECTED_WGRAD, f"weight-gradient families reached: {sorted(families)}, expected {sorted(EXPECTED_WGRAD)}"
    assert {4, 5} & families and {0, 1, 2, 3} & families, "F(2x3,3x3) and the direct tiles must both occur under zeros"
    # the split tiles of the implicit GEMM by the rule (rows without a forced split), and the forced 1 and 2
    by_rule = set().union(*(REACHED_SPLIT[r.id] for r in ROWS if r.split is None))
    assert by_rule & {2, 4}, f"no row took the split tiles by the rule: {sorted(by_rule)}"
    assert {1, 2} <= set().union(*REACHED_SPLIT.values())
