"""The planned kernel families of the zero-padded 3x3 rows (tests/test_conv_zero_pad_gpu.py) against that table, without a GPU,
as tests/test_conv_plan_rect.py does for the rectangle rows; and the plane sizes at which a zero-padded whole model reaches the
Winograd families, which is why tests/test_models_ctor_gpu.py runs 16 x 16, 32 x 32 and one 64 x 64 case."""
import ctypes

import pytest

import conv_trace as T
from crop2seg_amd import _lib
from crop2seg_amd import engine as E
from test_conv_zero_pad_gpu import N, ROWS


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in ("WINOGRAD", "WINO16", "S2WINO", "CONV_MODE"):      # whatever the C2S_* environment says
        monkeypatch.setattr(E, name, T.DEFAULTS[name])
    E.lib().c2s_wgrad_algorithms(-1, -1)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_planned_family_is_the_table_s(monkeypatch, row):
    monkeypatch.setattr(E, "CONV_MODE", row.conv_mode)
    monkeypatch.setattr(E, "WINO16", row.wino16)
    args = (N, row.chans, row.Cout, row.H, row.W, 3, 1, 1, _lib.PAD_ZEROS)
    fwd = E.conv_plan("fwd", *args)
    dgrad = [E.conv_plan("dgrad", *args, si=si, accumulate=a) for si, a in enumerate(row.acc)]
    assert fwd.family == row.fwd
    assert tuple(p.family for p in dgrad) == row.dgrad
    for plan, acc in zip(dgrad, row.acc):
        assert [(launch.desc.accumulate, launch.desc.reflect_adjoint) for launch in plan.launches] == [(acc, 0)]
    fam = ctypes.c_int(-1)
    d = E.WgradDesc(N, row.chans[0], sum(row.chans[1:]), row.H, row.W, row.Cout, row.H, row.W, 3, 3, 1, 1, 1, _lib.PAD_ZEROS, 4)
    assert E.lib().c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == 0      # (the family does not depend on nslices)
    assert fam.value == row.wgrad


@pytest.mark.parametrize("hw,s2,wino", [(16, ("igemm", "xpair"), "wino4"), (32, ("igemm", "xpair"), "wino16"),
                                        (64, ("s2wino", "s2dgrad"), "wino16")])
def test_whole_model_planes_under_zeros(hw, s2, wino):
    """The 64 -> 64 layers of a default-width encoder on B * T = 8 frames: the 3x3 layers run the 4-wave Winograd kernel at
    16 x 16 and the 8-wave one from 32 x 32; the 4x4 stride-2 pair takes F(2x2,2x2) from 64 x 64 only."""
    args = (8, [64], 64, hw, hw)
    assert (E.conv_plan("fwd", *args, 4, 2, 1, _lib.PAD_ZEROS).family, E.conv_plan("dgrad", *args, 4, 2, 1, _lib.PAD_ZEROS).family) == s2
    assert E.conv_plan("fwd", *args, 3, 1, 1, _lib.PAD_ZEROS).family == wino
    assert E.conv_plan("dgrad", *args, 3, 1, 1, _lib.PAD_ZEROS).family == wino
