"""tests/wgrad_ref.py checked without a GPU: the float32 model of the split-K walk meets the per-element bound against the
float64 references at every slice count and frame pattern, each way the walk can go wrong is rejected by that bound, and
every row of the table reaches the kernel family it names (c2s_wgrad_path, a host-only query) at every slice count."""
import ctypes
import types

import pytest
import torch

import conv_ref as R
import wgrad_ref as G
from crop2seg_amd import _lib
from crop2seg_amd import engine as E

CTX = types.SimpleNamespace(cus=256)          # what engine._wgrad_desc reads of a context
MODEL_ROWS = [r for r in G.ROWS if r.id in ("tile32-3x3", "tile32-4x4s2")]
_CACHE = {}


def _fixture(row):
    """(x, gout, frame references, float32 tiles, frame of every tile) of a row, computed once and left unchanged."""
    if row.id not in _CACHE:
        x, gout = G.make_inputs(row)
        tiles32, frames = G.tile_wgrads(row, x, gout, torch.float32)
        _CACHE[row.id] = (x, gout, G.frame_refs(row, x, gout), tiles32, frames)
    return _CACHE[row.id]


def _check(row, nslices, pattern, mutation=None):
    _, _, refs, tiles32, frames = _fixture(row)
    keep = G.keep_mask(pattern, row.N)
    got, applied = G.splitk_model(row, tiles32, frames, keep, nslices, mutation)
    assert applied == (mutation is not None), f"{mutation} does not apply to {row.id} nslices {nslices} pattern {pattern}"
    ref, A = G.pattern_ref(refs, keep)
    return lambda: R.assert_within(f"{row.id} nslices {nslices} {pattern}", got, ref, A, G.model_constant(row, nslices),
                                   R.FROB_GRAD)


def test_model_rows_are_a_3x3_and_a_4x4_stride_2():
    assert sorted((r.K, r.S) for r in MODEL_ROWS) == [(3, 1), (4, 2)]


@pytest.mark.parametrize("row", G.ROWS, ids=[r.id for r in G.ROWS])
def test_frame_counts(row):
    """One slice walks six tiles or more, each of two slices three or more, and 64 slices are more than the tiles."""
    nt = G.ntiles(row)
    assert 6 <= nt < 64
    assert all(len(G.walk(row, s, 2, nt)) >= 3 for s in range(2))
    for nslices in G.NSLICES:                 # every tile is walked once, with the permuted start too
        assert sorted(t for s in range(nslices) for t in G.walk(row, s, nslices, nt)) == list(range(nt))
    for pattern in G.PATTERNS:
        assert G.keep_mask(pattern, row.N).sum() == row.N - len(G.padded_frames(pattern, row.N))


def test_frame_patterns():
    assert G.padded_frames("none", 6) == [] and G.padded_frames("all", 3) == [0, 1, 2]
    assert G.padded_frames("tail", 6) == [1, 2, 5] and G.padded_frames("tail", 3) == [1, 2]
    assert G.padded_frames("head", 6) == [0, 4] and G.padded_frames("head", 3) == [0, 1]


@pytest.mark.parametrize("row", MODEL_ROWS, ids=[r.id for r in MODEL_ROWS])
def test_tiles_add_up_to_the_frames(row):
    """float64: the tiles of a frame (gout zeroed outside the tile) sum to the frame's weight gradient."""
    x, gout, (gw, A), _, frames = _fixture(row)
    tiles64, frames64 = G.tile_wgrads(row, x, gout, torch.float64)
    assert frames64 == frames and len(frames) == G.ntiles(row)
    per = len(frames) // row.N
    for n in range(row.N):
        assert frames[n * per:(n + 1) * per] == [n] * per
        err = (tiles64[n * per:(n + 1) * per].sum(0) - gw[n]).abs()
        assert bool((err <= 8 * 2.0 ** -53 * A[n] + 1e-300).all())


@pytest.mark.parametrize("pattern", G.PATTERNS)
@pytest.mark.parametrize("nslices", G.NSLICES)
@pytest.mark.parametrize("row", MODEL_ROWS, ids=[r.id for r in MODEL_ROWS])
def test_model_meets_the_bound(row, nslices, pattern):
    ratio = _check(row, nslices, pattern)()
    if pattern == "all":
        assert ratio == 0.0


# (nslices, pattern) at which each mutation has something to change
MUTATION_CASES = {
    "drop-last-tile": [(1, "none"), (3, "tail"), (8, "head"), (64, "none")],
    "drop-tile-after-skip": [(1, "tail"), (2, "tail"), (5, "tail"), (2, "head"), (3, "head"), (5, "head")],
    "tile-twice": [(1, "none"), (5, "tail"), (16, "head")],
    "padded-frame-included": [(1, "tail"), (3, "head"), (8, "tail"), (64, "head"), (3, "all")],
    "slab-left-out": [(1, "none"), (2, "tail"), (5, "head"), (64, "none")],
    "stale-empty-slab": [(16, "none"), (64, "tail"), (64, "head")],
}


def test_every_mutation_has_cases():
    assert sorted(MUTATION_CASES) == sorted(G.MUTATIONS)


@pytest.mark.parametrize("mutation,nslices,pattern", [(m, n, p) for m, cases in MUTATION_CASES.items() for n, p in cases])
@pytest.mark.parametrize("row", MODEL_ROWS, ids=[r.id for r in MODEL_ROWS])
def test_mutations_are_rejected(row, mutation, nslices, pattern):
    check = _check(row, nslices, pattern, mutation)          # (asserts that the mutation changed something)
    with pytest.raises(AssertionError):
        check()


def _family(row, nslices):
    pm = _lib.PAD_REFLECT if row.mode == "reflect" else _lib.PAD_ZEROS
    Ho, Wo = G.out_plane(row)
    srcs = [torch.empty(row.N, c, row.H, row.W, device="meta") for c in row.chans]
    d = E._wgrad_desc(CTX, srcs, row.Cout, Ho, Wo, row.K, row.S, row.pad, pm)
    d.nslices = nslices
    fam = ctypes.c_int(-1)
    assert _lib.lib().c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == 0, _lib.lib().c2s_last_error()
    return fam.value


def test_rows_reach_their_families():
    """Every row, at every slice count and under its forced algorithms, is on the family it names; together the rows reach
    the seven families and the fifteen instantiations."""
    L = _lib.lib()
    reached = set()
    try:
        for row in G.ROWS:
            L.c2s_wgrad_algorithms(*row.force)
            for nslices in G.NSLICES:
                assert _family(row, nslices) == row.family, (row.id, nslices)
            reached.add((row.family, row.K))
    finally:
        L.c2s_wgrad_algorithms(-1, -1)
    assert {f for f, _ in reached} == set(range(7))
    assert reached == G.INSTANTIATIONS and len(G.INSTANTIATIONS) == 15
    assert len({r.id for r in G.ROWS}) == len(G.ROWS)
