"""engine.conv_plan, the one place that chooses a convolution's kernel family, checked without a GPU: the launches of
conv2d / conv_transpose2d against the trace recorded before the plan existed (tests/conv_trace.py), the planned family of
every row of test_conv_paths_gpu.ROWS and of the two tables of test_conv_modes_gpu against the tables', and the frame-count
bounds of the choice."""
import json
import os

import pytest

import conv_trace as T
from crop2seg_amd import _lib
from crop2seg_amd import engine as E
from test_conv_modes_gpu import PERSISTENT, TABLES, persistent_frames
from test_conv_paths_gpu import ROWS

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_launch_trace.json")) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in ("WINOGRAD", "WINO16", "S2WINO", "CONV_MODE"):      # whatever the C2S_* environment says
        monkeypatch.setattr(E, name, T.DEFAULTS[name])


def test_the_grid_is_the_recorded_one():
    assert sorted(c["id"] for c in T.GRID) == sorted(GOLDEN)


@pytest.mark.parametrize("case", T.GRID, ids=[c["id"] for c in T.GRID])
def test_launch_trace_is_the_recorded_one(case):
    """Same entry points, descriptors, numbers, taps, packed weights and tensor roles, in the same order, under every switch
    setting."""
    assert T.record_case(case) == GOLDEN[case["id"]]


def _plan(op, N, chans, Cout, H, W, K, S, mode, **kw):
    pm = _lib.PAD_REFLECT if mode == "reflect" else _lib.PAD_ZEROS
    return E.conv_plan(op, N, chans, Cout, H, W, K, S, 0 if K == 1 else 1, pm, **kw)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_planned_family_is_the_table_s(row):
    args = (row.N, row.chans, row.Cout, row.H, row.W, row.K, row.S, row.mode)
    fwd = _plan("fwd", *args).family
    assert {"smallcin": "igemm"}.get(fwd, fwd) == row.fwd
    dgrad = tuple(_plan("dgrad", *args, si=si, accumulate=acc).family for si, acc in enumerate(row.acc))
    assert dgrad == row.dgrad


@pytest.mark.parametrize("mode,row", TABLES, ids=[r.id for _, r in TABLES])
def test_planned_family_of_the_mode_rows(mode, row, monkeypatch):
    """The first-layer and bf16x3 tables of test_conv_modes_gpu under their CONV_MODE; "smallcin" by its own name."""
    monkeypatch.setattr(E, "CONV_MODE", mode)
    args = (row.N, row.chans, row.Cout, row.H, row.W, row.K, row.S, row.mode)
    assert _plan("fwd", *args).family == row.fwd
    dgrad = tuple(_plan("dgrad", *args, si=si, accumulate=acc).family for si, acc in enumerate(row.acc))
    assert dgrad == row.dgrad


def test_the_persistent_row_outruns_the_grid():
    """first-persistent on 256 compute units: more tiles than the 2 * 256 workgroups of the first-layer kernel's grid, so
    workgroups reach a second tile; planned on that kernel."""
    N, padded = persistent_frames(256)
    row = PERSISTENT
    tiles = N * (row.H // 8) * (row.W // 32)
    assert (N, tiles) == (160, 640) and tiles > 2 * 256
    assert padded == [1, 3, 4, 5, 6, 10, 136, 137, 138, 159]
    assert _plan("fwd", N, row.chans, row.Cout, row.H, row.W, row.K, row.S, row.mode).family == "smallcin"


def test_frame_count_bounds():
    """The 8-wave Winograd kernel takes at most 65536 frames, the F(2x2,2x2) data gradient 32768."""
    wide = (64,), 64, 64, 64, 3, 1, "reflect"
    for op in ("fwd", "dgrad"):
        assert _plan(op, 65536, *wide).family == "wino16"
        assert _plan(op, 65537, *wide).family == "wino4"
    down = (64,), 64, 128, 128, 4, 2, "reflect"
    assert _plan("dgrad", 32768, *down).family == "s2dgrad"
    assert _plan("dgrad", 32769, *down).family == "xpair"
    assert [l.key for l in _plan("dgrad", 32769, *down).launches] == [("dgrad", 0, 0), ("dgrad", 0, 1)]


def test_switches_are_read_when_the_plan_is_made(monkeypatch):
    wide = (3, (64,), 64, 64, 64, 3, 1, "reflect")
    assert _plan("fwd", *wide).family == "wino16"
    monkeypatch.setattr(E, "WINO16", False)
    assert _plan("fwd", *wide).family == "wino4"
    monkeypatch.setattr(E, "WINOGRAD", False)
    assert _plan("fwd", *wide).family == "igemm"
    monkeypatch.setattr(E, "CONV_MODE", "bf16x3")
    assert _plan("fwd", *wide).family == "bf16x3"
    down = (3, (64,), 64, 128, 128, 4, 2, "reflect")
    monkeypatch.setattr(E, "CONV_MODE", "f32")
    assert (_plan("fwd", *down).family, _plan("dgrad", *down).family) == ("s2wino", "s2dgrad")
    monkeypatch.setattr(E, "S2WINO", False)
    assert (_plan("fwd", *down).family, _plan("dgrad", *down).family) == ("igemm", "xpair")
