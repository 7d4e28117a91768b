"""The depthwise dispatch as a pure host query (no GPU): c2s_dwconv_paths against the literals of tests/dw_ref.py and at the
neighbours of every boundary of its table (include/c2s_hip.h), the arguments it refuses, and the reference the GPU rows are
held to: its float32 evaluation stays within each row's constants of the float64 one, and its reflect data gradient on a
3x3 plane is the hand-summed one (five terms per dimension at the centre)."""
import ctypes

import pytest
import torch

import conv_ref as R
import dw_ref as D
from test_conv_split import LAYERS


def _L():
    from crop2seg_amd import _lib
    return _lib


# =================================================================================================
# dispatch
# =================================================================================================
@pytest.mark.parametrize("row", D.ROWS, ids=D.IDS)
def test_row_literal_is_the_reported_triple(row):
    assert D.row_paths(_L(), row) == row.paths


def test_rows_reach_both_variants_and_the_mixed_triples():
    """What the closing test of the GPU file asserts, from the literals alone."""
    for geom in D.REACHED_BOTH:
        triples = {r.paths for r in D.ROWS if (r.K, r.S, r.pad) == geom}
        for i in range(3):
            assert {t[i] for t in triples} == {1, 4}, (geom, i)
        assert D.MIXED[geom] <= triples
    assert all(r.paths == (1, 1, 1) for r in D.ROWS if r.K in (2, 6))


def test_boundary_neighbours():
    L = _L()
    p = lambda H, W, K, S, pad, mode="reflect": D.paths(L, H, W, K, S, pad, mode)
    # (3,1,1): the data gradient's stencil needs Win >= 8 and Hin >= 4
    assert p(8, 4, 3, 1, 1) == (4, 1, 4) and p(8, 8, 3, 1, 1) == (4, 4, 4)
    assert p(3, 8, 3, 1, 1) == (4, 1, 4) and p(4, 8, 3, 1, 1) == (4, 4, 4)
    assert p(8, 12, 3, 1, 1) == (4, 4, 4) and p(8, 10, 3, 1, 1) == (1, 1, 1)
    # (4,2,1): ... and an even Hin
    assert p(5, 16, 4, 2, 1) == (4, 1, 4) and p(6, 16, 4, 2, 1) == (4, 4, 4)
    assert p(3, 16, 4, 2, 1) == (4, 1, 4) and p(4, 16, 4, 2, 1) == (4, 4, 4) and p(2, 16, 4, 2, 1) == (4, 1, 4)
    # the span loader's precondition: Win = 9 has Wo = 4 and rows that are 4-byte aligned only
    assert p(8, 9, 4, 2, 1) == (1, 1, 1) and p(8, 8, 4, 2, 1) == (4, 4, 4)
    assert p(8, 6, 4, 2, 1) == (1, 1, 1)                                     # Wo = 3
    assert p(8, 12, 4, 2, 1) == (1, 4, 1)                                    # Wo = 6: only the stencil takes it
    assert p(8, 4, 4, 2, 1) == (1, 1, 1) and p(8, 17, 4, 2, 1) == (1, 1, 1)  # Wo = 2; Win odd, Wo = 8
    # the padding mode does not enter
    for H, W, K, S in ((8, 4, 3, 1), (3, 8, 3, 1), (5, 16, 4, 2), (8, 9, 4, 2), (4, 8, 4, 2)):
        assert p(H, W, K, S, 1, "zeros") == p(H, W, K, S, 1)
    # (2,2,0) and (6,2,2): one pixel per thread, always
    for K, pad in ((2, 0), (6, 2)):
        for H in (3, 4, 8, 9, 16, 64):
            for W in (3, 4, 8, 9, 16, 64):
                for mode in ("reflect", "zeros"):
                    assert p(H, W, K, 2, pad, mode) == (1, 1, 1), (K, H, W, mode)


def test_query_is_the_documented_table():
    """Every plane of 1..20 x 1..40 against the table at the declaration, written out here."""
    L = _L()
    for K, S in ((3, 1), (4, 2)):
        for H in range(2, 21):
            for W in range(2, 41):
                Wo = (W + 2 - K) // S + 1
                span = 4 if Wo % 4 == 0 and W % 4 == 0 else 1
                sten = 4 if W % 4 == 0 and W >= 8 and H >= 4 and (K == 3 or H % 2 == 0) else 1
                for mode in ("reflect", "zeros"):
                    assert D.paths(L, H, W, K, S, 1, mode) == (span, sten, span), (K, H, W, mode)


def test_no_even_plane_changed_its_kernel():
    """The forward / weight-gradient predicate was Wo % 4 == 0 alone; with Win % 4 == 0 added only odd widths of 4x4/s2 move
    (to one pixel per thread).  Over the plane sizes of the layer table of test_conv_split.py, and over every even width."""
    L = _L()
    sizes = sorted({hw for _, _, hw, _, _ in LAYERS})
    assert sizes == [4, 16, 32, 64, 128]
    planes = [(h, w) for h in sizes for w in sizes] + [(8, w) for w in range(2, 258, 2)]
    for K, S in ((3, 1), (4, 2)):
        for H, W in planes:
            before = 4 if ((W + 2 - K) // S + 1) % 4 == 0 else 1
            f, _, g = D.paths(L, H, W, K, S, 1)
            assert (f, g) == (before, before), (K, H, W)
        moved = [W for W in range(3, 259, 2) if ((W + 2 - K) // S + 1) % 4 == 0 and D.paths(L, 8, W, K, S, 1)[0] == 1]
        assert moved == ([] if K == 3 else list(range(9, 259, 8))), (K, moved)


def test_refused_arguments():
    lib = _L().lib()
    L = _L()
    f, d, g = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    out = (ctypes.byref(f), ctypes.byref(d), ctypes.byref(g))
    for K, S, pad in ((5, 1, 2), (3, 2, 1), (3, 1, 0), (4, 2, 0), (2, 2, 1), (6, 2, 1), (1, 1, 0)):
        assert lib.c2s_dwconv_paths(8, 8, K, S, pad, L.PAD_REFLECT, *out) == -1, (K, S, pad)
        assert b"(3,1,1), (4,2,1), (2,2,0) and (6,2,2)" in lib.c2s_last_error()
    for H, W, K, S, pad in ((1, 8, 3, 1, 1), (8, 1, 3, 1, 1), (1, 8, 4, 2, 1), (2, 8, 6, 2, 2), (8, 2, 6, 2, 2)):      # Hin <= pad
        assert lib.c2s_dwconv_paths(H, W, K, S, pad, L.PAD_REFLECT, *out) == -1, (H, W, K)
        assert b"reflect needs pad < plane" in lib.c2s_last_error()
    assert lib.c2s_dwconv_paths(2, 8, 6, 2, 2, L.PAD_ZEROS, *out) == 0                    # zero padding has no such limit
    assert lib.c2s_dwconv_paths(0, 8, 3, 1, 1, L.PAD_ZEROS, *out) == -1 and b"bad shape" in lib.c2s_last_error()
    assert lib.c2s_dwconv_paths(8, 8, 3, 1, 1, L.PAD_ZEROS, None, None, None) == -1
    assert b"null pointer" in lib.c2s_last_error()


def test_abi_version_unchanged():
    assert _L().lib().c2s_abi_version() == 4


# =================================================================================================
# the reference
# =================================================================================================
@pytest.mark.parametrize("row", D.ROWS, ids=D.IDS)
def test_fp32_evaluation_of_row_stays_within_its_constants(row):
    """torch's float32 evaluation of the row on the CPU (another fp32 order of the same sums) meets the per-element bound and
    the Frobenius bars the kernel is held to: the reference alone does not ask more than fp32 gives."""
    t = D.inputs(row)
    c = D.constants(row)
    keep, w, b = t["keep"], t["w"], t["b"]
    gw64 = gw32 = Agw = 0
    for x, gout, prior in t["calls"]:
        r = D.refs(row, x, w, b, gout, prior, keep)
        assert all(bool(torch.isfinite(v).all()) for v in r.values()), "a padded frame leaked into the reference"
        e = D.evaluate(row, x, w, b, gout, prior, keep, torch.float32)
        R.assert_within(f"{row.id} forward", e["y"], r["y"], r["Ay"], c["fwd"], R.FROB_FWD)
        R.assert_within(f"{row.id} data gradient", e["gx"], r["gx"], r["Agx"], c["dgrad"], R.FROB_GRAD)
        gw64, gw32, Agw = gw64 + r["gw"], gw32 + e["gw"], Agw + r["Agw"]
    R.assert_within(f"{row.id} weight gradient", gw32, gw64, Agw, c["wgrad"], R.FROB_GRAD)


def test_evaluate_in_float64_is_the_reference():
    row = next(r for r in D.ROWS if r.id == "k3-h3")
    t = D.inputs(row)
    x, gout, prior = t["calls"][0]
    r = D.refs(row, x, t["w"], None, gout, prior, t["keep"])
    e = D.evaluate(row, x, t["w"], None, gout, prior, t["keep"], torch.float64)
    assert all(torch.equal(e[k], r[k]) for k in ("y", "gx", "gw"))


def test_reflect_data_gradient_on_a_3x3_plane_is_the_hand_sum():
    """Centre pixel of a 3x3 plane under 3x3/s1 reflect padding.  Per dimension, input index 1 is read by output o through tap
    k where o - 1 + k is 1 (directly: three pairs), -1 or 3 (the two padded positions, which both mirror onto 1): five pairs,
    25 terms in the plane.  A corner has 2 x 2 and an edge centre 2 x 5."""
    row = next(r for r in D.ROWS if r.id == "k3-3x3")
    t = D.inputs(row)
    x, gout, _ = t["calls"][0]
    keep, w = t["keep"], t["w"]
    gx = D.refs(row, x, w, None, gout, None, keep)["gx"]
    pairs = {0: [(0, 1), (1, 0)], 1: [(2, 0), (1, 1), (0, 2), (0, 0), (2, 2)], 2: [(2, 1), (1, 2)]}
    assert len(pairs[1]) == 5
    g64, w64 = gout[keep].double(), w.double()
    for n in range(int(keep.sum())):
        for ch in range(D.C):
            for jy in range(3):
                for jx in range(3):
                    s = sum(w64[ch, 0, ky, kx] * g64[n, ch, oy, ox] for oy, ky in pairs[jy] for ox, kx in pairs[jx])
                    assert abs(float(gx[n, ch, jy, jx] - s)) <= 1e-13 * (1 + abs(float(s))), (n, ch, jy, jx)
