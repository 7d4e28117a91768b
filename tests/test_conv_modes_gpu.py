"""The first-layer kernel (conv_first.hip, family "smallcin") and the split-precision kernel (conv_bf16x3.hip, family
"bf16x3", engine.CONV_MODE = "bf16x3") against the float64 references of tests/conv_ref.py, element by element.

The conventions are those of test_conv_paths_gpu.py: N >= 3 with padded frames (valid[n] = 0) whose x and gout are NaN; an
accumulated prior gradient holds the sentinel 1234.5 on the padded frames, which must still be bit-identical after the
backward pass; the weight gradient must be finite; every result also meets the Frobenius bars.  The kernel that ran is
observed with a spy around engine._run_conv, which records (family, forward / data gradient, source, accumulate,
reflect_adjoint) of every launch: "smallcin" and "igemm" pack their weights alike, so the pack keys cannot tell them apart.

Table A (FIRST_ROWS, CONV_MODE = "f32"): the channel counts 10, 9, 5, 4 and 1 (masked channels of the last pair), both
paddings, the second block of 64 output channels, the data gradient into 10 channels on the implicit GEMM with a prior, and
two neighbours the kernel's predicate must refuse.  test_first_layer_persistent_loop has more tiles than the 2 * CUs
workgroups of the persistent grid, so workgroups walk to a second tile: padded frames are placed so that a workgroup meets
"first tile padded, second real", "first real, second padded", "both padded", four padded frames in a row and a padded
last frame.

Table B (BF16X3_ROWS, CONV_MODE = "bf16x3"): accumulate together with the in-kernel reflect adjoint, frame widths 32, 16,
8 and 4, a 2 x 2 plane (adjoint range ay_hi < ay_lo), the wide kernel (MF = 2) with padded output channels, zero padding
(no adjoint), two sources, and Cout = 15 whose data gradient stays on the implicit GEMM.

Bounds, |got - ref64| <= bound element by element, A = the same map on absolute values (+ |prior|):

    smallcin, igemm     C_FAMILY["igemm"] * 2^-24 * A          (the same v_mfma_f32_32x32x2_f32 accumulation)
    bf16x3              (2^-16 + C_FAMILY["igemm"] * 2^-24) * A

The first bf16x3 term is derived: with round-to-nearest bf16 splits |v - hi - lo| <= 2^-18 |v| and |lo| <= 2^-9 |v|, so the
two split residuals and the dropped lo * lo term sum to at most 3 * 2^-18 |a||b| < 2^-16 |a||b| per product; the second
term is the fp32 accumulation.  Frobenius bars: conv_ref.FROB_FWD / FROB_GRAD for smallcin, igemm and the weight gradients
(which stay on the exact fp32 kernels in both modes), 5e-5 for bf16x3 results (the bar of test_ops_gpu.py).

Observed worst ratios max |err| / (u * A) on an MI355X (printed with -s), u = 2^-24 for smallcin / igemm / the weight
gradients and u = 2^-16 for bf16x3:

    smallcin 5.51   igemm 5.13   bf16x3 0.13   wgrad_direct 3.11   wgrad_f23 1.43

The rows can fail (local builds, not part of the project, each run once; both change values only, never an address):
- conv_first.hip with the prefetch condition changed to frame_ok(tile): test_first_layer_persistent_loop fails (forward
  Frobenius error 1.3e-1: stale patches behind padded frames) while the nine rows of Table A and every CONV_CASES row of
  test_ops_gpu.py still pass;
- conv_bf16x3.hip with the accumulate add of the epilogue skipped: the nine rows of Table B that accumulate through that
  kernel fail (bx and bx-cout15, whose accumulating data gradient runs on the implicit GEMM, pass) while
  test_conv3x3_bf16x3_fwd_bwd still passes.
"""
import math

import pytest
import torch

import conv_ref as R
from test_conv_paths_gpu import C_FAMILY, SENTINEL, Row, _check_wgrad, _ctx, _gen, _keep, _observed_wgrad, _randn
from test_conv_paths_gpu import EXPECTED_WGRAD as PATHS_WGRAD

pytestmark = pytest.mark.gpu

U_BF16X3 = 2.0 ** -16
FROB_BF16X3 = 5e-5                  # the bar of test_ops_gpu.test_conv3x3_bf16x3_fwd_bwd
# family -> (c in units of u = 2^-24, Frobenius bar forward, Frobenius bar gradient, u of the printed ratio)
BOUNDS = {
    "smallcin": (C_FAMILY["igemm"], R.FROB_FWD, R.FROB_GRAD, R.U),
    "igemm": (C_FAMILY["igemm"], R.FROB_FWD, R.FROB_GRAD, R.U),
    "bf16x3": (U_BF16X3 / R.U + C_FAMILY["igemm"], FROB_BF16X3, FROB_BF16X3, U_BF16X3),
}
OBSERVED = {}           # family -> worst max |err| / (u * A), u of the family
REACHED = {}            # row id -> set of (family, op, accumulate, reflect_adjoint)
REACHED_WGRAD = {}      # row id -> set of weight-gradient families (c2s_wgrad_path)

# Table A.  Row of test_conv_paths_gpu; an empty `dgrad` means E.conv2d(..., need_input_grad=False), as functional.py
# calls the first layer.  All rows are 3x3 stride 1 with a bias.  The last field is the weight-gradient family
# c2s_wgrad_path reports.
FIRST_ROWS = [
    Row("first-10", 3, (10,), 64, 32, 64, 3, 1, "reflect", (), "smallcin", (), 3),
    Row("first-10-zeros", 3, (10,), 64, 32, 64, 3, 1, "zeros", (), "smallcin", (), 3),
    # one tile per frame (top and bottom reflection in one patch), odd channel count, blockIdx.y reaches 1
    Row("first-9-two-blocks", 3, (9,), 128, 8, 32, 3, 1, "reflect", (), "smallcin", (), 3),
    Row("first-5", 3, (5,), 64, 16, 32, 3, 1, "zeros", (), "smallcin", (), 3),     # NP = 5, five masked channels
    Row("first-4", 3, (4,), 64, 16, 64, 3, 1, "reflect", (), "smallcin", (), 3),   # NP = 2, full
    Row("first-1", 3, (1,), 64, 8, 32, 3, 1, "zeros", (), "smallcin", (), 3),      # NP = 2, three masked channels
    # the data gradient into 10 channels, added to a prior, with the reflect adjoint: implicit GEMM
    Row("first-10-dgrad-acc", 3, (10,), 64, 32, 32, 3, 1, "reflect", (1,), "smallcin", ("igemm",), 3),
    # neighbours the predicate refuses: 11 channels; a plane that is no multiple of the 8 x 32 tile
    Row("first-11", 3, (11,), 64, 16, 32, 3, 1, "reflect", (), "igemm", (), 1),
    Row("first-10-ragged-plane", 3, (10,), 64, 20, 36, 3, 1, "reflect", (), "igemm", (), 0),
]

# Table B.  The weight gradient of every row stays on the exact fp32 kernels.
BF16X3_ROWS = [
    Row("bx", 3, (64,), 64, 64, 64, 3, 1, "reflect", (0,), "bf16x3", ("bf16x3",), 5),
    Row("bx-acc", 3, (64,), 64, 64, 64, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 5),          # ADJ + accumulate
    Row("bx-5frames-acc", 5, (64,), 64, 16, 16, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 2),  # FC = 16, two padded frames
    # forward CoutP = 96 (MF = 1, three blocks); data gradient into 32 channels; partial tiles both ways
    Row("bx-ragged-acc", 3, (32,), 72, 12, 40, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 0),
    # CoutP = 64: MF = 2 with 24 padded output channels; data gradient from 40 channels (5 chunks)
    Row("bx-cout40-acc", 3, (64,), 40, 24, 40, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 0),
    Row("bx-two-sources-acc-skip", 3, (32, 64), 64, 32, 64, 3, 1, "reflect", (0, 1), "bf16x3", ("bf16x3", "bf16x3"), 4),
    Row("bx-8wide-acc", 3, (128,), 128, 8, 8, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 0),    # FC = 8
    Row("bx-4x4-acc", 3, (128,), 128, 4, 4, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 0),      # FC = 4: all border
    Row("bx-2x2-acc", 3, (64,), 64, 2, 2, 3, 1, "reflect", (1,), "bf16x3", ("bf16x3",), 0),        # ay_hi < ay_lo
    Row("bx-zeros-acc", 3, (40,), 64, 8, 32, 3, 1, "zeros", (1,), "bf16x3", ("bf16x3",), 5),       # no adjoint
    Row("bx-cout15", 3, (32,), 15, 32, 32, 3, 1, "reflect", (1,), "bf16x3", ("igemm",), 1),        # Cout % 8 != 0: igemm dgrad
]

TABLES = [("f32", r) for r in FIRST_ROWS] + [("bf16x3", r) for r in BF16X3_ROWS]

PERSISTENT = Row("first-persistent", 0, (10,), 64, 32, 32, 3, 1, "reflect", (), "smallcin", (), 3)   # N: persistent_frames(cus)


def persistent_frames(cus):
    """(N, padded frames) of first-persistent for a device with `cus` compute units.  The kernel launches
    min(ntiles, 2 * cus) workgroups and a 32 x 32 plane has 4 tiles, so F = 2 * cus // 4 frames fill one pass of the grid
    and a workgroup that starts in frame k goes on in frame k + F.  N = F + F // 4; relative to (k, k + F) the padded
    frames cover: first padded and second real (1, 3, 4, 5, 6: also four padded frames in a row), first real and second
    padded (F + 8, F + 9), both padded (10 and F + 10), and a padded last frame."""
    F = 2 * cus // 4
    N = F + F // 4
    return N, sorted({1, 3, 4, 5, 6, F + 8, F + 9, 10, F + 10, N - 1})


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _spy(m, E):
    """Wrap engine._run_conv: every launch is recorded as (family, "fwd" / "dgrad", source index, accumulate,
    reflect_adjoint) and the call is forwarded unchanged."""
    calls, real = [], E._run_conv

    def run_conv(ctx, plan, *args, **kw):
        for launch in plan.launches:
            op = launch.key[0]
            calls.append((plan.family, op, launch.key[-1] if op == "dgrad" else None, launch.desc.accumulate,
                          launch.desc.reflect_adjoint))
        return real(ctx, plan, *args, **kw)

    m.setattr(E, "_run_conv", run_conv)
    return calls


def _note(family, ratio24):
    """ratio24 = max |err| / (2^-24 * A); recorded in the u of the family."""
    ratio = ratio24 * R.U / BOUNDS[family][3]
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), ratio)
    return ratio


def _run_row(mode, row, monkeypatch, keep=None):
    E, L = _engine()
    g = _gen(row.id)
    N, K, S, pad = row.N, 3, 1, 1
    pm = L.PAD_REFLECT if row.mode == "reflect" else L.PAD_ZEROS
    radj = int(row.mode == "reflect")
    Cin, H, W = sum(row.chans), row.H, row.W
    keep = _keep(N) if keep is None else keep
    need_input_grad = bool(row.dgrad)
    x = _randn((N, Cin, H, W), g, keep)
    w = torch.randn(row.Cout, Cin, K, K, generator=g) / math.sqrt(Cin * K * K)
    b = torch.randn(row.Cout, generator=g)
    gout = _randn((N, row.Cout, H, W), g, keep)
    prior = torch.zeros_like(x)
    ctx = _ctx({"w": w, "b": b})
    srcs, lo = [], 0
    for si, c in enumerate(row.chans):
        srcs.append(x[:, lo:lo + c].contiguous().cuda())
        if need_input_grad and row.acc[si]:
            p = _randn((N, c, H, W), g, keep, SENTINEL)
            prior[:, lo:lo + c] = p
            ctx.tape.grads[srcs[-1].data_ptr()] = p.cuda()
        lo += c
    vd, gd = keep.int().cuda(), gout.cuda()
    with monkeypatch.context() as m:                # the mode and the spy end with the row
        m.setattr(E, "CONV_MODE", mode)
        calls = _spy(m, E)
        out = E.conv2d(ctx, srcs, "w", "b", K, S, pad, pm, vd, need_input_grad=need_input_grad)
        ctx.tape.grads[out.data_ptr()] = gd
        ctx.tape.backward()
        torch.cuda.synchronize()
        wk = _observed_wgrad(ctx, srcs, gd, row.Cout, H, W, K, S, pad, pm, Cin * K * K, K * K, list(range(K * K)), vd,
                             ctx.g["w"])
    # the kernels that ran
    fwd = [c for c in calls if c[1] == "fwd"]
    dgrad = sorted((c for c in calls if c[1] == "dgrad"), key=lambda c: c[2])
    assert len(calls) == len(fwd) + len(dgrad) and len(fwd) == 1, f"{row.id}: launches {calls}"
    assert fwd[0] == (row.fwd, "fwd", None, 0, 0), f"{row.id}: forward launch {fwd[0]}, the table says {row.fwd}"
    want = [(k, "dgrad", si, a, radj) for si, (k, a) in enumerate(zip(row.dgrad, row.acc))]
    assert dgrad == want, f"{row.id}: data-gradient launches {dgrad}, the table says {want}"
    REACHED_WGRAD[row.id] = {_check_wgrad(row.id, ctx, srcs, row.Cout, H, W, K, S, pad, pm, wk, row.wgrad)}
    REACHED[row.id] = {(c[0], c[1], c[3], c[4]) for c in calls} | {(wk, "wgrad", 0, 0)}

    # the values
    ref = R.conv_refs(x[keep], w, b, gout[keep], S, pad, row.mode)
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
    OBSERVED[wk] = max(OBSERVED.get(wk, 0.0), q)
    print(f"\n{row.id}: " + "  ".join(shown) + f"  {wk} {q:.2f}")


@pytest.mark.parametrize("row", FIRST_ROWS, ids=[r.id for r in FIRST_ROWS])
def test_first_layer(row, monkeypatch):
    _run_row("f32", row, monkeypatch)


@pytest.mark.parametrize("row", BF16X3_ROWS, ids=[r.id for r in BF16X3_ROWS])
def test_bf16x3(row, monkeypatch):
    _run_row("bf16x3", row, monkeypatch)


def _run_persistent(monkeypatch):
    E, _ = _engine()
    cus = E.lib().c2s_device_cus()
    N, padded = persistent_frames(cus)
    tiles_per_frame = (PERSISTENT.H // 8) * (PERSISTENT.W // 32)
    assert tiles_per_frame == 4 and 4 * N > 2 * cus, f"{4 * N} tiles do not exceed the {2 * cus} workgroups of the grid"
    keep = torch.ones(N, dtype=torch.bool)
    keep[padded] = False
    _run_row("f32", PERSISTENT._replace(N=N), monkeypatch, keep)


def test_first_layer_persistent_loop(monkeypatch):
    """More tiles than workgroups: the second iteration of the persistent loop, with the prefetch handed over between
    real and padded frames in every order (persistent_frames)."""
    _run_persistent(monkeypatch)


# =================================================================================================
# coverage: the paths the tables reached
# =================================================================================================
EXPECTED = {
    ("smallcin", "fwd", 0, 0), ("igemm", "fwd", 0, 0), ("bf16x3", "fwd", 0, 0),
    ("bf16x3", "dgrad", 0, 1), ("bf16x3", "dgrad", 1, 1), ("bf16x3", "dgrad", 1, 0),
    ("igemm", "dgrad", 1, 1),
    ("wgrad_direct", "wgrad", 0, 0), ("wgrad_f23", "wgrad", 0, 0),
}
EXPECTED_WGRAD = {0, 1, 2, 3, 4, 5}      # (6, the 4x4 stride-2 form, is reached by test_conv_paths_gpu.py)


def test_reached_paths_are_the_table(monkeypatch):
    """Every (family, op, accumulate, reflect_adjoint) and every weight-gradient family the tables reached, against the
    expected sets: a dispatch change that moves a row to another kernel fails its row, one that drops a path altogether fails
    here.  Rows not run yet in this session (-k selections) run here."""
    for mode, row in TABLES:
        if row.id not in REACHED:
            _run_row(mode, row, monkeypatch)
    if PERSISTENT.id not in REACHED:
        _run_persistent(monkeypatch)
    reached = set().union(*REACHED.values())
    print("\nworst |err| / (u * A) per kernel family: " + "  ".join(f"{k} {v:.2f}" for k, v in sorted(OBSERVED.items())))
    assert reached == EXPECTED, f"missing {sorted(EXPECTED - reached)}, unexpected {sorted(reached - EXPECTED)}"
    families = set().union(*REACHED_WGRAD.values())
    assert families == EXPECTED_WGRAD, f"weight-gradient families reached: {sorted(families)}, expected {sorted(EXPECTED_WGRAD)}"
    assert EXPECTED_WGRAD | PATHS_WGRAD == set(range(7)), "the two tables together reach every weight-gradient family"
