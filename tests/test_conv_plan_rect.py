"""The planned kernel families of the rectangle rows (tests/test_conv_rect_gpu.py) against that table, without a GPU, as
tests/test_conv_plan.py does for the square tables; and the plan of 3-pixel planes, which every arithmetic mode keeps on the
implicit GEMM with the reflect adjoint folded in (conv_igemm.hip takes them; the bf16x3 kernel's adjoint does not)."""
import ctypes

import pytest

import conv_trace as T
from crop2seg_amd import _lib
from crop2seg_amd import engine as E
from test_conv_rect_gpu import ROWS, ROWS_3PX, UP, UP_WGRAD


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in ("WINOGRAD", "WINO16", "S2WINO", "CONV_MODE"):      # whatever the C2S_* environment says
        monkeypatch.setattr(E, name, T.DEFAULTS[name])
    E.lib().c2s_wgrad_algorithms(-1, -1)


def _wgrad_family(C0, C1, Hin, Win, Cout, Ho, Wo, K, S, pad, pm):
    fam = ctypes.c_int(-1)
    d = E.WgradDesc(3, C0, C1, Hin, Win, Cout, Ho, Wo, K, K, S, pad, pad, pm, 4)     # (the family does not depend on nslices)
    assert E.lib().c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == 0
    return fam.value


@pytest.mark.parametrize("row", ROWS + ROWS_3PX, ids=[r.id for r in ROWS + ROWS_3PX])
def test_planned_family_is_the_table_s(row):
    pm = _lib.PAD_REFLECT if row.mode == "reflect" else _lib.PAD_ZEROS
    args = (row.N, row.chans, row.Cout, row.H, row.W, row.K, row.S, 1, pm)
    assert E.conv_plan("fwd", *args).family == row.fwd
    assert tuple(E.conv_plan("dgrad", *args, si=si, accumulate=a).family for si, a in enumerate(row.acc)) == row.dgrad
    Ho, Wo = (row.H + 2 - row.K) // row.S + 1, (row.W + 2 - row.K) // row.S + 1
    assert _wgrad_family(row.chans[0], sum(row.chans[1:]), row.H, row.W, row.Cout, Ho, Wo, row.K, row.S, 1, pm) == row.wgrad


@pytest.mark.parametrize("K,pad,cin,cout,H,W,acc", UP)
def test_transposed_weight_gradient_family(K, pad, cin, cout, H, W, acc):
    assert _wgrad_family(cout, 0, 2 * H, 2 * W, cin, H, W, K, 2, pad, _lib.PAD_ZEROS) == UP_WGRAD.get((K, H, W), 0)
    plan = E.conv_plan("tfwd", 2, [cin], cout, H, W, K, 2, pad, _lib.PAD_ZEROS)
    assert plan.family == ("xpair" if K == 4 else "parity")
    for launch in plan.launches:
        d = launch.desc
        assert (d.Hin, d.Win, d.Hout, d.Wout, d.OutH, d.OutW) == (H, W, H, W, 2 * H, 2 * W)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("H,W", [(3, 8), (8, 3), (3, 3), (3, 32)])
def test_three_pixel_planes_plan_onto_the_implicit_gemm(monkeypatch, mode, H, W):
    monkeypatch.setattr(E, "CONV_MODE", mode)
    for op in ("fwd", "dgrad"):
        plan = E.conv_plan(op, 3, [64], 64, H, W, 3, 1, 1, _lib.PAD_REFLECT)
        assert plan.family == "igemm"
        assert plan.launches[0].desc.reflect_adjoint == (1 if op == "dgrad" else 0)
