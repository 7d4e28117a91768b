"""Existing rows inside the guard-band arena of tests/redzone.py: stores outside a tensor, elements never stored, and reads
of memory nobody initialised.

Every case runs the runner of an existing GPU test UNCHANGED (its fp64 bounds, sentinels and path assertions included)
while every device allocation of torch's factories is a block between poisoned guard bands and `empty` memory is a NaN
pattern.  After the runner: the guard bands are intact (arena.__exit__), and no allocation made inside crop2seg_amd/ still
holds poison, except where include/c2s_hip.h says nothing is written (FRAMES, SCRATCH and `may_keep` below).  That covers
group_stats, row_ab, the L-TAE's stats, pooled / hidden / scale and the parcel tables without naming them.

Wrapped rows and the boundary each one puts inside a tensor:

    test_conv_paths_gpu.ROWS     wino16-ragged-acc, wino16-ragged-dgrad-acc (12 x 40: partial Winograd tiles both ways; 72
                                 channels: a half-empty block of 64), wino4-ragged-acc, wino4-ragged-dgrad-acc (36 channels),
                                 two-sources-acc-skip (two packed weights, two gradients), igemm-cout32 (Cout < the 64-wide
                                 tile), igemm-4x4-acc (plane smaller than a tile), igemm-1x1-acc, s2-ragged-acc (F(2x2,2x2)
                                 on 12 x 40 outputs, 8 -> 72 channels), xpair-acc (16-wide output rows)
    TRANSPOSE_SHAPES             (2,128,64,4,4), (2,64,32,16,16): the parity launches at the narrowest planes
    test_conv_rect_gpu           wino4-2x8 (one row of Winograd tiles), igemm-8x2-acc, xpair-16x4-acc (2-wide output of the
                                 data gradient's source plane), 3px-64ch-3x3-acc, the K = 6 transposed convolution on 2 x 8:
                                 thin planes, where an access outside the plane shows first
    DEPTHWISE                    hw 6 (one output per thread) and 40 x 48 (float4 spans), (K,S) = (3,1) and (4,2)
    test_strided_geometry DOWN   (72,40,24,1) and (64,64,4,1), reflect, geometries (2,2,0) and (6,2,2): ragged channels both
                                 ways; a 2 x 2 output plane
    test_strided_geometry UP     (72,40,8,0), (128,64,4,1), both geometries
    test_dw_reference_gpu        k3-h3, k3-w3, k3-3x3, k3-2x2, k4-odd-h, k4-odd-w: 3-pixel, 2-pixel and odd-width planes
    test_conv_modes_gpu          first-10 on one 8 x 32 tile per frame (the smallest plane conv_first.hip takes; the row of
                                 the table with H, W replaced); bx-cout40-acc (24 padded output channels), bx-ragged-acc
    test_wgrad_slices_gpu        one row per family 0 - 6 at nslices 5 (12 or 24 tiles: the last slices walk a tile fewer), 64
                                 (more slices than tiles: empty slabs) and 3 with accumulate, slab workspace and destination
                                 sized by the query
    test_conv_split_gpu          3x3-cin36-20x36 at split 2 and 4 (tile overhang both ways)
    norm_ref rows                one-pass: g_nk1 (flags), g_nk2_res (flags + residual), b_nk2_res, g_frozen_producer_nk4
                                 (gx == NULL); two-pass: b_flags, b_flags_3x3, b_flags_47, g_3x3, g_5x5_res,
                                 g_47_unaligned_res (row bases 4-byte aligned only), g_frozen_producer_5x5, g_noaffine_3x3;
                                 each on a fresh Workspace inside the arena (sync area included)
    SE, pixel GN                 every row; aggregation: att_mean_accumulate, mean
    test_agg_adjoint_gpu         ratio8, padded_frame_prior_gattn, tiled_plane
    test_s2dgrad_skip_gpu        partial_tiles, cs48_csp64, one_padded_frame, fused path only (asserted)
    test_tail_reference_gpu      ce_hw257_k15, focal_hw257_k15 (771 pixels), smooth_batch_edge, the first reduction="none"
                                 row, adam_n257_off3, adam_n255_off1, metrics_k15_blocks (1311 pixels), boundary_2x12x17
    test_guard_gpu               the SMALL slot table (padding between slots): adam_slots clipped, grad_sumsq
    outside engine.py            label_components, parcel_vote and parcel_soft_vote through postprocess.py; cut_windows and
                                 softmax_blend + blend_finish on 10 x 21 (smaller than a window) and 37 x 45 (clamped last
                                 window, W % 4 != 0); softmax_stitch with crop 41 of 48; SeriesCollator staged, uint16
    new row                      the collator on uint16 values in 32768 .. 65535, staged and zero_copy, also outside the arena
    L-TAE (child processes)      px16_c256_t31_hw20, lds_c128_t39, t1, t64, acc_abs_rel_doy, rng_lds_8px_p0.1,
                                 reg_fwd_lds_bwd_noemb, rng_reg_noattn_p0.5, stream_hw8_t13, acc_reg; no_lds: px16_c64_t9;
                                 stream: rng_stream_p0.5; long: t65_c64_hw32, t129_c256_offset; hparams: h8_dv32_partial,
                                 h16_dv32_t.  Families reached inside the arena (asserted): forward 0 - 4, backward 0 - 6
    whole steps                  one eager TrainStep with apply_update=True of UTAE, TimeUNet_v1, WTAE, UTAE(use_mbconv=True),
                                 UTAE(add_squeeze_excit=True, conv_type="depthwise_separable") and UTAE with the guarded
                                 update (clipping): bit-identical to the same step under the ordinary allocator in loss,
                                 logits, flat_grad, flat_param, both Adam moments, every buffer (and the guard's status block
                                 and step counts); sync_error() == 0

The Adam, metrics and guard runners write into tensors they made with `.cuda()`; those cases run with copies=True, which
gives such copies blocks of their own.

Found by these rows: nothing to fix.  On an MI355X no guard band was damaged in any case, every whole step was bit-identical,
and poison survived only where the header says nothing is written: the padded frames of convolution outputs, of fresh data
gradients and of pooled / hidden / scale (one frame in three or four, whole frames only), `out` of the two parcel votes at
labels outside [0, cap] (1727 of 8192 pixels with cap = 3; 2 pixels), and the unused part of one-dimensional workspaces
(for example 76032 of the 110592 floats of the weight-gradient workspace of the first-layer row, 352 of 496 floats of a
normalisation workspace).  One refusal on the way: the collator's kernel takes planes with HW % 4 == 0 only and returned
its error code for a first draft of the uint16 row on 9 x 7 pixels, as rule 2 of the header asks; the row uses 6 x 10.

Wall time on an MI355X: profiles/redzone_times.txt (every case with and without the arena; the arena adds its fill and
its scan, a few milliseconds; the L-TAE groups cost what their child processes cost).
"""
import json
import os
import subprocess
import sys
import time
from typing import Callable, NamedTuple, Tuple

import numpy as np
import pytest
import torch

import redzone as RZ

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB = 1 << 20


class Case(NamedTuple):
    id: str
    run: Callable                  # run(monkeypatch): the runner of an existing test, unchanged
    may_keep: Tuple[str, ...] = ()  # "function:dtype" of further allocations that may hold poison after this case
    mib: int = 256                 # arena size
    copies: bool = False           # the runner's kernels write into tensors it made with .cuda(): give those blocks too


# Allocations of crop2seg_amd/ that may still hold poison after a row, by allocating function (include/c2s_hip.h):
# - FRAMES: "padded frames are skipped".  Outputs [N, ...] of the convolutions, fresh data gradients and the per-frame
#   vectors of squeeze-and-excitation are not written on frames with valid == 0.  Poison may cover whole frames only, and
#   never every frame; the runners check every real frame by value, where poison is a NaN.
# - SCRATCH: one-dimensional workspaces (Workspace.get, the normalisation backward's partial sums).  A query may ask for
#   more than a launch fills; whatever a consumer reads of it ends in an output that the runner checks.
# - per case (may_keep): `out` of the parcel votes at labels outside [0, cap].
# Everything else the engine allocates inside the arena must be overwritten completely.
FRAMES = ("conv2d", "depthwise_conv2d", "grad_buffer", "squeeze_excite")
SCRATCH = ("get", "bwd")

CASES = []


def case(id, run, may_keep=(), mib=256, copies=False):
    CASES.append(Case(id, run, tuple(may_keep), mib, copies))


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _function(site):
    return site.rsplit("(", 1)[1].rstrip(")")


def residue_allowed(a, b, may_keep=()):
    """Block `b` of arena `a` still holds poison: is that one of the cases above?"""
    fn, t = _function(b.site), a.tensor(b)
    if f"{fn}:{str(b.dtype).replace('torch.', '')}" in may_keep:
        return True
    if fn in SCRATCH:
        return t.dim() == 1
    if fn in FRAMES and t.dim() >= 2 and t.dtype.itemsize == 4:
        rows = a.poisoned(t).reshape(t.shape[0], -1)
        return bool((rows.all(1) | ~rows.any(1)).all()) and not bool(rows.all())
    return False


def in_arena(c: Case, monkeypatch):
    """The case's runner inside the arena: its own assertions hold on poisoned uninitialised memory, the guard bands are
    intact afterwards (__exit__), and no allocation of the engine still holds poison where it should have been written."""
    t0 = time.perf_counter()
    with RZ.arena("cuda", c.mib * MB, copies=c.copies) as a:
        c.run(monkeypatch)
        torch.cuda.synchronize()
        left = a.unwritten()
        bad = [(b, n) for b, n in left if not residue_allowed(a, b, c.may_keep)]
    dt = time.perf_counter() - t0
    print(f"\n{c.id}: {len(a.blocks)} blocks, {a.allocated} bytes in {a.used} of the arena, {dt:.3f} s; poison left in "
          f"{[(_function(b.site), b.shape, n) for b, n in left]}")
    assert not bad, f"{c.id}: outputs still holding poison: " + "; ".join(f"{b} ({n} words)" for b, n in bad)
    return a


# =================================================================================================
# convolutions
# =================================================================================================
def _conv_cases():
    import dw_ref as D
    import test_conv_modes_gpu as CM
    import test_conv_paths_gpu as CP
    import test_conv_rect_gpu as CR
    import test_conv_split_gpu as CS
    import test_dw_reference_gpu as DW
    import test_strided_geometry_gpu as SG
    import test_wgrad_slices_gpu as WS
    import wgrad_ref as G

    for rid in ("wino16-ragged-acc", "wino16-ragged-dgrad-acc", "wino4-ragged-acc", "wino4-ragged-dgrad-acc",
                "two-sources-acc-skip", "igemm-cout32", "igemm-4x4-acc", "igemm-1x1-acc", "s2-ragged-acc", "xpair-acc"):
        row = next(r for r in CP.ROWS if r.id == rid)
        case(f"conv/{rid}", lambda mp, row=row: CP._run_row(row))
    for shape in ((2, 128, 64, 4, 4), (2, 64, 32, 16, 16)):
        assert shape in CP.TRANSPOSE_SHAPES
        case(f"transpose/{'x'.join(map(str, shape))}", lambda mp, shape=shape: CP._run_transpose(shape))
    # one thin-plane row per family of test_conv_rect_gpu.py, and the 3 x 3 plane whose two reflected rows fold onto one
    for rid in ("rect-wino4-2x8", "rect-igemm-8x2-acc", "rect-xpair-16x4-acc", "rect-3px-64ch-3x3-acc"):
        row = next(r for r in CR.ROWS + CR.ROWS_3PX if r.id == rid)
        case(f"conv/{rid}", lambda mp, row=row: CR._run(row))
    assert (6, 2, 128, 64, 2, 8, 1) in CR.UP
    case("up/rect-k6-128-64-2x8", lambda mp: CR.test_conv_transpose_rect(6, 2, 128, 64, 2, 8, 1))
    for K, S, hw in CP.DEPTHWISE:
        if hw in (6, 40):
            case(f"depthwise/k{K}s{S}-{hw}", lambda mp, a=(K, S, hw): CP._run_depthwise(*a))
    for K, pad in SG.GEOMS:
        for cin, cout, hw, acc in ((72, 40, 24, 1), (64, 64, 4, 1)):
            assert (K, pad, "reflect", cin, cout, hw, acc) in SG.DOWN
            case(f"down/k{K}-{cin}-{cout}-{hw}", lambda mp, a=(K, pad, "reflect", cin, cout, hw, acc): SG.test_down_conv(*a))
        for cin, cout, hw, acc in ((72, 40, 8, 0), (128, 64, 4, 1)):
            assert (K, pad, cin, cout, hw, acc) in SG.UP
            case(f"up/k{K}-{cin}-{cout}-{hw}", lambda mp, a=(K, pad, cin, cout, hw, acc): SG.test_conv_transpose(*a))
    for rid in ("k3-h3", "k3-w3", "k3-3x3", "k3-2x2", "k4-odd-h", "k4-odd-w"):
        row = next(r for r in D.ROWS if r.id == rid)
        case(f"dw/{rid}", lambda mp, row=row: DW._run_row(row))
    # the first layer on the smallest plane its kernel takes (one 8 x 32 tile per frame), and bf16x3 with ragged Cout
    first = next(r for r in CM.FIRST_ROWS if r.id == "first-10")._replace(id="first-10-8x32", H=8, W=32)
    case("modes/first-10-8x32", lambda mp: CM._run_row("f32", first, mp))
    for rid in ("bx-cout40-acc", "bx-ragged-acc"):
        row = next(r for r in CM.BF16X3_ROWS if r.id == rid)
        case(f"modes/{rid}", lambda mp, row=row: CM._run_row("bf16x3", row, mp))

    def wgrad(row):
        def run(mp):
            E, _ = _engine()
            E.Workspace(torch.device("cuda"))
            try:
                E.lib().c2s_wgrad_algorithms(*row.force)
                c = WS._Case(row)
                assert G.ntiles(row) % 5 != 0 and G.ntiles(row) < 64
                c.check(5, "tail")                 # the last slices walk one tile fewer
                c.check(64, "none")                # more slices than tiles: empty slabs
                c.check(3, "tail", accumulate=1)
            finally:
                E.lib().c2s_wgrad_algorithms(-1, -1)
        return run
    for rid in ("generic-3x3-ragged", "tile32-3x3", "tile16-3x3", "first-10", "f23-4wave-two-sources", "f23-8wave", "f22"):
        row = next(r for r in G.ROWS if r.id == rid)
        case(f"wgrad/{rid}", wgrad(row))
    split = next(c for c in CS.CASES if c.id == "3x3-cin36-20x36")
    for sp in (2, 4):
        case(f"split/{split.id}-x{sp}", lambda mp, sp=sp: CS.test_forced_split(split, sp, mp))


# =================================================================================================
# normalisation, squeeze-and-excitation, aggregation
# =================================================================================================
def _norm_cases():
    import norm_ref as R
    import test_agg_adjoint_gpu as AA
    import test_norm_reference_gpu as NR
    import test_s2dgrad_skip_gpu as SK

    def norm(name):
        def run(mp):
            E, _ = _engine()
            mp.setitem(NR._SHARED, "ws", E.Workspace(torch.device("cuda")))      # a fresh workspace, inside the arena
            NR.test_norm_rows_per_element(name, mp)
        return run
    names = {r["name"] for r in R.norm_rows(256)}
    for name in ("g_nk1", "g_nk2_res", "g_frozen_producer_nk4", "b_nk2_res", "b_flags", "b_flags_3x3", "b_flags_47", "g_3x3",
                 "g_5x5_res", "g_47_unaligned_res", "g_frozen_producer_5x5", "g_noaffine_3x3"):
        assert name in names
        case(f"norm/{name}", norm(name))
    for r in R.se_rows():
        case(f"se/{r['name']}", lambda mp, n=r["name"]: NR.test_se_rows_per_element(n))
    for name in ("att_mean_accumulate", "mean"):
        case(f"agg/{name}", lambda mp, n=name: NR.test_agg_rows_per_element(n))
    for r in R.pixel_gn_rows():
        case(f"pixel_gn/{r['name']}", lambda mp, n=r["name"]: NR.test_pixel_gn_rows_per_element(n))
    for name in ("ratio8", "padded_frame_prior_gattn", "tiled_plane"):
        case(f"agg_adjoint/{name}", lambda mp, n=name: AA.test_agg_adjoint_rows_per_element(n))

    def skip(name):
        def run(mp):
            *shape, kw = SK.CASES[name]
            _, n1 = SK.run(mp, True, *shape, **kw)
            assert n1.get("c2s_temporal_aggregate_bwd_skip") == 1 and n1.get("c2s_conv4x4s2_dgrad_winograd_skip") == 1
        return run
    for name in ("partial_tiles", "cs48_csp64", "one_padded_frame"):
        case(f"s2dgrad_skip/{name}", skip(name))


# =================================================================================================
# losses, Adam, metrics, the guarded step's entry points
# =================================================================================================
def _tail_cases():
    import test_guard_gpu as GD
    import test_tail_reference_gpu as TR

    def row(rows, name):
        return next(r for r in rows if r["name"] == name)
    px = lambda r: r["B"] * r["H"] * r["W"]      # noqa: E731
    ce, focal = row(TR.CE_ROWS, "ce_hw257_k15"), row(TR.FOCAL_ROWS, "focal_hw257_k15")
    smooth = [row(TR.SMOOTH_ROWS, "smooth_batch_edge"), next(r for r in TR.SMOOTH_ROWS if r.get("reduction") == "none")]
    metric, boundary = row(TR.METRIC_ROWS, "metrics_k15_blocks"), row(TR.BOUNDARY_ROWS, "boundary_2x12x17")
    assert all(px(r) % 256 for r in [ce, focal, metric, boundary] + smooth)
    case(f"tail/{ce['name']}", lambda mp: TR.test_cross_entropy(ce))
    case(f"tail/{focal['name']}", lambda mp: TR.test_focal_ce(focal))
    for r in smooth:
        case(f"tail/{r['name']}", lambda mp, r=r: TR.test_smooth_ce(r))
    for name in ("adam_n257_off3", "adam_n255_off1"):                     # n % 4 != 0 at offsets 3 and 1
        case(f"tail/{name}", lambda mp, r=row(TR.ADAM_ROWS, name): TR.test_adam(r), copies=True)
    case(f"tail/{metric['name']}", lambda mp: TR.test_metrics_update(metric), copies=True)
    case(f"tail/{boundary['name']}", lambda mp: TR.test_boundary_and_region(boundary))
    case("guard/adam_slots-clipped", lambda mp: GD.test_adam_slots_against_adam_ref(0.37, 0.125), copies=True)
    case("guard/grad_sumsq-small", lambda mp: GD.test_grad_sumsq(GD.SMALL, "normal"), copies=True)


# =================================================================================================
# outside engine.py: parcels, raster windows, stitch, collator
# =================================================================================================
def collate_uint16_above_int16(mode):
    """uint16 reflectances above 32767 (the rows of test_tail_gpu.py draw below 12000): a kernel that reads the series as
    int16 turns them negative."""
    import test_tail_gpu as TG
    from crop2seg_amd.utils import CHANNELS_LIKE_PASTIS, SeriesCollator
    rng = np.random.default_rng(3)
    lengths = [3, 5, 1]
    series = [rng.integers(32768, 65536, (t, 10, 6, 10)).astype(np.uint16) for t in lengths]     # 60 pixels
    series[1][0, :, 0, 0], series[1][1, :, 0, 0] = 65535, 32768
    dates = [np.sort(rng.integers(1, 400, t)).astype(np.int64) for t in lengths]
    mean, std = rng.normal(40000, 300, 10), rng.uniform(300, 900, 10)
    x, dd, valid = SeriesCollator(CHANNELS_LIKE_PASTIS, mean, std, mode=mode)(series, dates)
    rx, rd = TG.TO.collate_series(series, dates, CHANNELS_LIKE_PASTIS, mean, std)
    assert torch.equal(x.cpu(), rx) and torch.equal(dd.cpu(), rd)
    assert valid.view(3, 5).cpu().tolist() == [[1] * t + [0] * (5 - t) for t in lengths]
    raw, _, _ = SeriesCollator(None, None, None, mode=mode)(series, dates)
    assert float(raw[1, 0, :, 0, 0].min()) == 65535.0 and float(raw[1, 1, :, 0, 0].max()) == 32768.0


def _outside_cases():
    import parcel_soft_ref as SR
    import test_parcel_gpu as PG
    import test_parcel_soft_gpu as PS
    import test_raster_gpu as RG
    import test_tail_gpu as TG
    case("parcels/label_components", lambda mp: PG.test_label_components_python_entry())
    # its last call votes with cap = 3 on ids up to the scene's maximum: `out` is not written above the cap
    case("parcels/vote", lambda mp: PG.test_homogenize_end_to_end(), ("_vote:int64",))
    case("parcels/soft_vote", lambda mp: PS.test_homogenize_soft_is_the_soft_vote(SR.make_soft_scene(2, 16, 96, 100, seed=61)))
    # labels outside [0, cap]: `out` is not written there (include/c2s_hip.h), and the Python entry does not prefill it
    case("parcels/soft_vote-skipped", lambda mp: PS.test_empty_ids_and_skipped_pixels(), ("parcel_soft_vote:int64",))
    for hw, stride in (((10, 21), 12), ((37, 45), 12)):                   # smaller than one window; a clamped last window
        assert (hw, stride) in RG.GEOMETRIES
        case(f"raster/cut-{hw[0]}x{hw[1]}", lambda mp, a=(hw, stride): RG.test_cut_windows_bit_exact(*a))
        case(f"raster/blend-finish-{hw[0]}x{hw[1]}",
             lambda mp, a=(hw, stride, "hann"): RG.test_blend_matches_fp64_and_is_batch_invariant(*a))
    case("stitch/crop41-of-48", lambda mp: TG.test_softmax_stitch_matches_restatement())
    case("collate/staged-uint16", lambda mp: TG.test_collate_series_bit_exact(np.uint16, "staged"))
    for mode in ("staged", "zero_copy"):
        case(f"collate/{mode}-uint16-above-32767", lambda mp, mode=mode: collate_uint16_above_int16(mode))


_conv_cases()
_norm_cases()
_tail_cases()
_outside_cases()
assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_row_in_arena(c, monkeypatch):
    in_arena(c, monkeypatch)


def test_collate_uint16_above_int16_plain():
    """The new collator row outside the arena too (it is no row of another file)."""
    for mode in ("staged", "zero_copy"):
        collate_uint16_above_int16(mode)


# =================================================================================================
# L-TAE: the rows run in child processes (the C2S_LTAE_* switches are read once per process)
# =================================================================================================
LTAE_MIB = 2048          # per row; the largest (rng_reg_noattn_p0.5, which runs twice) uses 859 MiB
LTAE_SEEN = {}           # group -> {row name: ROW record}


def _ltae_groups():
    import test_ltae_hparams_gpu as HP
    import test_ltae_long_gpu as LG
    import test_ltae_reference_gpu as TG

    def pick(rows, names):
        got = [r for r in rows if r["name"] in names]
        assert len(got) == len(names), names
        return got
    ref, ok, default = "ltae_ref_worker.py", "LTAE_REF_OK", TG.GROUPS["default"][0]
    groups = {
        # the rows on maps of 16 to 64 pixels, one process
        "default-small": (ref, ok, default, lambda: pick(TG.rows_default(), (
            "px16_c256_t31_hw20", "lds_c128_t39", "t1", "t64", "acc_abs_rel_doy", "rng_lds_8px_p0.1"))),
        "no_lds": (ref, ok, TG.GROUPS["no_lds"][0], lambda: pick(TG.rows_no_lds(), ("px16_c64_t9",))),
        "stream": (ref, ok, TG.GROUPS["stream"][0], lambda: pick(TG.rows_stream(), ("rng_stream_p0.5",))),
        "long": (ref, ok, {}, lambda: pick(LG.rows_long(), ("t65_c64_hw32", "t129_c256_offset"))),
        "hparams": ("ltae_hp_worker.py", "LTAE_HP_OK", {}, lambda: pick(HP.ROWS, ("h8_dv32_partial", "h16_dv32_t"))),
    }
    # the rows on maps that fill the chip, a process each (their float64 references take seconds).  acc_reg is the smallest
    # row of backward family 3 (register-resident, attn stored), which none of the other rows reports
    for name in ("reg_fwd_lds_bwd_noemb", "rng_reg_noattn_p0.5", "stream_hw8_t13", "acc_reg"):
        groups["default-" + name] = (ref, ok, default, lambda name=name: pick(TG.rows_default(), (name,)))
    return groups


LTAE_GROUPS = ["default-small", "default-reg_fwd_lds_bwd_noemb", "default-rng_reg_noattn_p0.5", "default-stream_hw8_t13",
               "default-acc_reg", "no_lds", "stream", "long", "hparams"]


def _run_ltae_group(group, mib=LTAE_MIB):
    """The group's rows in one child process, inside an arena of `mib` MiB each (0: as the other test files run them)."""
    import ltae_ref as R
    worker, ok, env_extra, rows = _ltae_groups()[group]
    rs = rows()
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", worker), json.dumps(rs), json.dumps(R.C_KERNEL)]
                       + ([str(mib)] if mib else []), env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=600)
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            res = json.loads(line[4:])
            seen[res["row"]] = res
            print({k: v for k, v in res.items() if k in ("row", "fwd", "bwd", "redzone", "unwritten", "arena_used")})
    print(f"ltae/{group}: {time.perf_counter() - t0:.1f} s")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert f"{ok} {len(rs)}" in r.stdout and set(seen) == {row["name"] for row in rs}
    if not mib:
        assert not any("redzone" in res for res in seen.values())
        return seen
    for name, res in seen.items():
        assert res["redzone"] == "intact", name
        bad = [u for u in res["unwritten"] if not (_function(u[0]) in SCRATCH and len(u[1]) == 1)]
        assert not bad, f"{name}: outputs still holding poison: {bad}"
    LTAE_SEEN[group] = seen
    return seen


@pytest.mark.parametrize("group", LTAE_GROUPS)
def test_ltae_rows_in_arena(group):
    _run_ltae_group(group)


def test_ltae_reached_every_family_in_the_arena():
    """Forward families 0 - 4 and backward families 0 - 6 of c2s_ltae_paths.  Groups not run yet in this session run here."""
    assert set(LTAE_GROUPS) == set(_ltae_groups())
    for group in LTAE_GROUPS:
        if group not in LTAE_SEEN:
            _run_ltae_group(group)
    reached = {(r["fwd"], r["bwd"]) for seen in LTAE_SEEN.values() for r in seen.values()}
    assert {f for f, _ in reached} == set(range(5)), reached
    assert {b for _, b in reached} == set(range(7)), reached


# =================================================================================================
# whole steps
# =================================================================================================
def _models():
    import crop2seg_amd as C2S
    return {
        "utae": (lambda: C2S.UTAE(input_dim=10, out_conv=[32, 15]), 15),
        "timeunet": (lambda: C2S.TimeUNet_v1(input_dim=10, out_conv=[32, 15]), 15),
        "wtae": (lambda: C2S.WTAE(input_dim=10, out_conv=[32, 15]), 15),
        # MBConv: c2s_channel_bias_add, squeeze-and-excitation and the depthwise convolution inside the block
        "utae_mbconv": (lambda: C2S.UTAE(input_dim=10, out_conv=[32, 20], use_mbconv=True), 20),
        "utae_se_dwsep": (lambda: C2S.UTAE(input_dim=10, out_conv=[32, 15], add_squeeze_excit=True,
                                           conv_type="depthwise_separable"), 15),
    }


STEP_MIB = 384           # the arena reports its use: 76 - 108 MiB per step, 242 MiB for MBConv (649 blocks), guard bands included
STEPS = [("utae", {}), ("timeunet", {}), ("wtae", {}), ("utae_mbconv", {}), ("utae_se_dwsep", {}),
         ("utae", dict(max_grad_norm=1e-3, skip_nonfinite=True))]
_STATE = {}


def _one_step(model, guard):
    """One eager TrainStep with apply_update=True from the seeded state; everything it leaves behind, on the CPU."""
    from crop2seg_amd.learning.utils import TrainStep
    from oracle import seeded
    make, K = _models()[model]
    net = make()
    if model not in _STATE:
        _STATE[model] = seeded.make_state([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 3, "tame")
    net.load_state_dict(_STATE[model])
    net = net.cuda().train()
    net.spec.attn_dropout = 0.0
    net.spec.mlp_dropout = 0.0
    x, dates, y = seeded.make_inputs(2, 3, 10, 32, 32, 91, [3, 2], n_classes=K)         # a padded frame in the second series
    step = TrainStep(net, num_classes=K, **guard)
    loss, logits = step(x.cuda(), dates.cuda(), y.cuda(), apply_update=True)
    torch.cuda.synchronize()
    out = {"loss": loss, "logits": logits, "flat_grad": step.flat_grad, "flat_param": step.flat_param, "exp_avg": step.exp_avg,
           "exp_avg_sq": step.exp_avg_sq}
    out.update({"buffer " + k: b for k, b in net.named_buffers()})
    if guard:
        out.update({"slot_steps": step.slot_steps_dev, "status": step._status})
        assert step.skipped_steps() == 0 and 0.0 < float(step.last_clip_coef) < 1.0, "the guard must clip, not skip"
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    assert step.ws.sync_error() == 0, "a one-pass normalisation wait gave up"
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


@pytest.mark.parametrize("model,guard", STEPS, ids=[m + ("-guarded" if g else "") for m, g in STEPS])
def test_train_step_in_arena_is_bit_identical(model, guard):
    """The same step from the same state outside and inside the arena: a difference means that some kernel's result depends on
    memory it did not write.  The guard bands must be intact; poison may stay wherever the step's own results do not read."""
    plain = _one_step(model, guard)
    t0 = time.perf_counter()
    with RZ.arena("cuda", STEP_MIB * MB) as a:
        inside = _one_step(model, guard)
    print(f"\nstep {model} {guard}: {len(a.blocks)} blocks, {a.allocated} bytes in {a.used} of the arena, "
          f"{time.perf_counter() - t0:.2f} s in the arena")
    assert set(plain) == set(inside)
    for k in plain:
        assert bool(torch.isfinite(plain[k].double()).all()), k
        assert plain[k].shape == inside[k].shape and torch.equal(_bits(plain[k]), _bits(inside[k])), \
            f"{model}: {k} differs between the ordinary allocator and the arena"


# =================================================================================================
# the harness itself on the device
# =================================================================================================
def test_device_write_past_the_end_is_reported():
    """A torch indexed write one element past the end of an arena tensor (the target lies inside the arena's own buffer): the
    exit check fails and names the block.  Nothing outside the arena's allocation is touched."""
    a = RZ.arena("cuda", 4 * MB)
    with pytest.raises(RZ.RedzoneError, match=r"block 1 \(5, 3\) float32.*past its end") as err:
        with a:
            torch.zeros(16, device="cuda")
            t = torch.zeros(5, 3, device="cuda")
            idx = torch.tensor([15], device="cuda")
            assert a.contains(t) and not a.contains(idx) and t.data_ptr() % 512 == 0
            assert a.base <= t.data_ptr() + 4 * 15 < a.base + a.nbytes - 4
            t.as_strided((16,), (1,), t.storage_offset()).index_fill_(0, idx, 1.0)
    assert "'+0'" in str(err.value) and "test_redzone_gpu.py" in str(err.value)
    e, = a.damage()
    assert e["block"].index == 1 and e["end"] == [0]


def test_device_arena_basics():
    """empty is NaN / poison on the device, zeros is zero, a clean kernel launch leaves the bands intact, copies=True puts
    `.cuda()` results into blocks, exhaustion raises before any launch."""
    E, L = _engine()
    with RZ.arena("cuda", 4 * MB, copies=True) as a:
        e = torch.empty(7, 3, device="cuda")
        z = torch.zeros(5, device="cuda", dtype=torch.int64)
        assert bool(a.poisoned(e).all()) and bool(e.isnan().all()) and bool((z == 0).all())
        up = torch.arange(6.0).cuda()
        assert a.contains(up) and not a.contains(torch.arange(6.0, device="cuda")) and up.cpu().tolist() == [0, 1, 2, 3, 4, 5]
        L.check(L.lib().c2s_fill(e.data_ptr(), e.numel(), 2.0, E._stream()), "fill")
        assert not bool(a.poisoned(e).any()) and bool((e == 2.0).all())
        assert a.unwritten("test_redzone_gpu") == []
    with pytest.raises(RZ.ArenaExhausted):
        with RZ.arena("cuda", MB):
            torch.empty(MB, device="cuda")
