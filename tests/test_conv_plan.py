"""engine.conv_plan, the one place that chooses a convolution's kernel family, checked without a GPU: the launches of
conv2d / conv_transpose2d against the trace recorded before the plan existed (tests/conv_trace.py), the planned family of
every row of test_conv_paths_gpu.ROWS and of the two tables of test_conv_modes_gpu against the tables', and the frame-count
bounds of the choice.  The weight gradient's family is chosen in the library (c2s_wgrad_path, a host-only query): the same rows
against the same tables, and the boundaries of that choice."""
import ctypes
import json
import os
import types

import pytest
import torch

import conv_trace as T
import test_conv_walk_gpu as W
from crop2seg_amd import _lib
from crop2seg_amd import engine as E
from test_conv_modes_gpu import PERSISTENT, TABLES, persistent_frames
from test_conv_paths_gpu import ROWS, TRANSPOSE_SHAPES, TRANSPOSE_WGRAD, WGRAD_TWICE, WGRAD_TWICE_FAMILY, wgrad_family

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


def test_the_walk_rows_outrun_the_grid():
    """The rows of test_conv_walk_gpu on 256 compute units: planned on the families of the table, and every workgroup of a ring
    launch's first grid pass reaches a third tile across every padded / real pattern (walk_frames asserts both)."""
    frames = {}
    for row in W.ROWS:
        N, padded = W.walk_frames(row, 256)
        frames[row.id] = (N, len(padded))
        args = (N, row.chans, row.Cout, row.H, row.W, row.K, row.S, row.mode)
        for acc in row.acc:
            assert (_plan("fwd", *args).family, _plan("dgrad", *args, accumulate=acc).family) == (row.fwd, row.dgrad[0])
    assert frames == {"wino16-walk": (208, 10), "wino16-walk-zeros": (208, 10), "wino16-walk-dgrad": (208, 10),
                      "wino16-walk-dgrad-zeros": (208, 10), "s2-walk": (416, 19), "s2-walk-k5": (416, 19)}
    assert W.ring_passes(W.ROWS[4], 256)[0] == [128, 32]       # s2wino: two tiles per frame; s2dgrad: four, and grid y = 2


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


# =================================================================================================
# the weight gradient: c2s_wgrad_path
# =================================================================================================
CTX = types.SimpleNamespace(cus=256)          # what engine._wgrad_desc reads of a context; as on an MI355X


def _wgrad(N, chans, Cout, Ho, Wo, K, S, pad=None, pm=_lib.PAD_REFLECT, Hin=None, Win=None):
    """Family of the launch engine._wgrad_launch makes; the input plane is S times the output plane unless given."""
    Hin, Win = Ho * S if Hin is None else Hin, Wo * S if Win is None else Win
    srcs = [torch.empty(N, c, Hin, Win, device="meta") for c in chans]
    return wgrad_family(CTX, srcs, Cout, Ho, Wo, K, S, (0 if K == 1 else 1) if pad is None else pad, pm)


def _wgrad_cases():
    """(id, expected family, arguments of _wgrad) of every weight gradient the two GPU tables launch by default."""
    cases = []
    for row in ROWS + [r for _, r in TABLES] + [PERSISTENT._replace(N=persistent_frames(256)[0])]:
        pad = 0 if row.K == 1 else 1
        Ho, Wo = (row.H + 2 * pad - row.K) // row.S + 1, (row.W + 2 * pad - row.K) // row.S + 1
        pm = _lib.PAD_REFLECT if row.mode == "reflect" else _lib.PAD_ZEROS
        cases.append((row.id, row.wgrad, dict(N=row.N, chans=row.chans, Cout=row.Cout, Ho=Ho, Wo=Wo, K=row.K, S=row.S, pad=pad,
                                              pm=pm, Hin=row.H, Win=row.W)))
    for shape in TRANSPOSE_SHAPES:            # dW of the transposed convolution: input = its gout, gout = its x
        N, Cin, Cout, H, W = shape
        cases.append((f"transpose{shape}", TRANSPOSE_WGRAD[shape],
                      dict(N=N, chans=(Cout,), Cout=Cin, Ho=H, Wo=W, K=4, S=2, pm=_lib.PAD_ZEROS)))
    for K, S, N, Cc, Cout, H, W in WGRAD_TWICE:
        cases.append((f"twice{K}{S}", WGRAD_TWICE_FAMILY[K, S][True],
                      dict(N=N, chans=(Cc,), Cout=Cout, Ho=(H + 2 - K) // S + 1, Wo=(W + 2 - K) // S + 1, K=K, S=S, Hin=H, Win=W)))
    return cases


def test_wgrad_path_query_without_gpu():
    """c2s_wgrad_path on every weight gradient of the GPU tables (the tables' own literals), under c2s_wgrad_algorithms, and one
    step either side of every boundary of the choice."""
    L = _lib.lib()
    cases = _wgrad_cases()
    assert len(cases) == len(ROWS) + len(TABLES) + 1 + 3 + 2
    for name, want, kw in cases:
        assert _wgrad(**kw) == want, name
    assert {want for _, want, _ in cases} == set(range(7))
    try:
        L.c2s_wgrad_algorithms(0, 0)
        for name, want, kw in cases:
            got = _wgrad(**kw)
            assert (got in (0, 1, 2) and got != want) if want >= 4 else got == want, (name, got)
        for K, S, N, Cc, Cout, H, W in WGRAD_TWICE:
            assert _wgrad(N, (Cc,), Cout, H // S, W // S, K, S) == WGRAD_TWICE_FAMILY[K, S][False]
        L.c2s_wgrad_algorithms(0, -1)          # each algorithm has its own switch
        assert (_wgrad(3, (64,), 64, 32, 32, 3, 1), _wgrad(3, (64,), 64, 32, 32, 4, 2)) == (1, 6)
        L.c2s_wgrad_algorithms(-1, 0)
        assert (_wgrad(3, (64,), 64, 32, 32, 3, 1), _wgrad(3, (64,), 64, 32, 32, 4, 2)) == (5, 1)
        L.c2s_wgrad_algorithms(-1, -1)
        for name, want, kw in cases:
            assert _wgrad(**kw) == want, name
    finally:
        L.c2s_wgrad_algorithms(-1, -1)

    f3 = lambda chans, Cout=64, Ho=32, Wo=32: _wgrad(3, chans, Cout, Ho, Wo, 3, 1)
    f4 = lambda chans, Cout=64, Ho=32, Wo=32: _wgrad(3, chans, Cout, Ho, Wo, 4, 2)
    f1 = lambda chans, Cout=64, Ho=32, Wo=32: _wgrad(3, chans, Cout, Ho, Wo, 1, 1)
    # families 4 - 6 need 32 input and 32 output channels
    assert (f3((32,), 32), f3((31,), 32), f3((32,), 31), f3((16, 16), 32), f3((16, 15), 32)) == (4, 1, 1, 4, 1)
    assert (f4((32,), 32), f4((28, 4), 32), f4((28, 3), 32), f4((32,), 31)) == (6, 6, 1, 1)
    # 5 where the input channels, rounded up to blocks of 32, are a multiple of 64
    assert [f3((c,)) for c in (33, 64, 65, 96, 97, 128)] == [5, 5, 4, 4, 5, 5]
    # the first-layer form up to 10 input channels, 3x3 only
    assert (f3((10,)), f3((11,)), f3((6, 4)), f3((6, 5)), f1((10,)), f4((8,))) == (3, 1, 3, 1, 1, 1)
    assert f3((10,), Wo=16) == 2 and f3((10,), Wo=48) == 0
    # plane width: 16 -> the 16-wide tiles, multiples of 32 -> the Winograd families or the 32-wide tiles, else generic
    assert [f3((64,), Wo=w) for w in (8, 16, 32, 48, 64)] == [0, 2, 5, 0, 5]
    assert [f4((64,), Wo=w) for w in (8, 16, 32, 48, 64)] == [0, 2, 6, 0, 6]
    assert [f1((64,), Wo=w) for w in (8, 16, 32, 48, 64)] == [0, 2, 1, 0, 1]
    # plane height: whole 4-row tiles for 4 - 6; whole tiles of 64 (128 for 1x1) positions for 1 - 3
    assert [f3((64,), Ho=h) for h in (28, 30, 31)] == [5, 1, 0] and [f3((64,), Ho=h, Wo=16) for h in (28, 30)] == [2, 0]
    assert [f4((64,), Ho=h) for h in (28, 30, 31)] == [6, 1, 0] and [f4((64,), Ho=h, Wo=16) for h in (28, 30)] == [2, 0]
    assert [f1((64,), Ho=h) for h in (28, 30)] == [1, 0] and [f1((64,), Ho=h, Wo=16) for h in (24, 28)] == [2, 0]
    # 6 reads the first source in float4 rows of channel quads
    assert (f4((32, 32)), f4((30, 34)), f4((34, 30))) == (6, 1, 1)
    # an input plane that is not S times the output plane (another padding) leaves only the generic kernel
    assert _wgrad(3, (64,), 64, 32, 32, 3, 1, pad=0, Hin=34, Win=34) == 0
    assert _wgrad(3, (64,), 64, 32, 32, 4, 2, pad=0, Hin=66, Win=66) == 0
    assert _wgrad(3, (64,), 64, 32, 32, 1, 1, pad=1, Hin=30, Win=30) == 0
    # 2x2 and 6x6 stride-2 layers have the generic kernel only
    for chans, Cout, Ho, Wo in (((64,), 64, 32, 32), ((64,), 64, 16, 16), ((10,), 64, 32, 64), ((32, 32), 128, 5, 7)):
        assert _wgrad(3, chans, Cout, Ho, Wo, 2, 2, pad=0) == 0 and _wgrad(3, chans, Cout, Ho, Wo, 6, 2, pad=2) == 0
    # what c2s_conv_wgrad refuses, the query refuses alike
    fam = ctypes.c_int(-7)
    d = _lib.WgradDesc(3, 64, 0, 32, 32, 64, 32, 32, 5, 5, 1, 2, 2, _lib.PAD_REFLECT, 4)
    assert L.c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == -1 and b"unsupported (K=5,S=1)" in L.c2s_last_error()
    d = _lib.WgradDesc(3, 64, 0, 32, 32, 64, 32, 32, 3, 1, 1, 1, 1, _lib.PAD_REFLECT, 4)
    assert L.c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == -1 and b"square kernels" in L.c2s_last_error()
    assert fam.value == -7
