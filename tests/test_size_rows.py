"""The size-edge rows of tests/size_rows.py without a GPU: their arithmetic in Python integers, the size queries at shapes
past 2^32, the kernel choice across each edge, and every refusal (the exports validate before they touch the device, so a
refusal row returns its message here exactly as it does on the GPU, with nothing launched).  test_size_limits_gpu.py runs
the launches."""
import ctypes

import pytest

import size_rows as Z


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _plan_args(L, s, N):
    pm = L.PAD_REFLECT if s["mode"] == "reflect" else L.PAD_ZEROS
    return (s["op"], N, list(s["chans"]), s["Cout"], s["H"], s["W"], s["K"], s["S"], s["pad"], pm)


def _desc_at(L, plan, N):
    d = L.ConvDesc.from_buffer_copy(plan.launches[0].desc)
    d.N = N
    return d


def _no_device():
    """The refusals are probed with placeholder pointers, so that a guard that regressed would launch on them: only where no
    device is present can that do no harm (hipLaunchKernel fails).  With a device the probes are left out."""
    import torch
    return not torch.cuda.is_available()


def _launch_unlaunched(L, family, d):
    """The family's entry point on placeholder pointers: only for descriptors the entry point must refuse (it validates
    before it touches the device), and only without a device (_no_device)."""
    assert _no_device()
    lib, p, ref = L.lib(), 16, ctypes.byref(d)
    if family in ("igemm", "parity"):
        return lib.c2s_conv_igemm(ref, p, None, p, None, p, None, None)
    if family == "xpair":
        return lib.c2s_conv_xpair(ref, p, p, None, p, None, None)
    if family == "bf16x3":
        return lib.c2s_conv3x3_bf16x3(ref, p, None, p, p, None, p, None, None)
    if family == "wino16":
        return lib.c2s_conv3x3_winograd16(ref, p, None, p, None, p, None, None)
    if family == "s2wino":
        return lib.c2s_conv4x4s2_winograd(ref, p, p, None, p, None, None)
    if family == "s2dgrad":
        return lib.c2s_conv4x4s2_dgrad_winograd(ref, p, p, p, None, None)
    raise AssertionError(family)


@pytest.mark.parametrize("row", Z.ROWS, ids=[r.id for r in Z.ROWS])
def test_row_arithmetic(row):
    """The crossing shape crosses, the shape below it does not, and no smaller count of the same shape crosses."""
    assert Z.crosses(row, row.cross), (row.id, Z.value(row, row.cross))
    at_refused_edge = row.expect == "refusal" and Z.value(row, row.below) > row.limit     # the 65,537 rows of the z families
    assert at_refused_edge or not Z.crosses(row, row.below), (row.id, Z.value(row, row.below))
    assert Z.value(row, row.below) < Z.value(row, row.cross)
    if row.quantity == "planes":
        for s in (row.cross, row.below):
            assert Z.DW_COUNTS[s["N"] * s["C"]] == (s["N"], s["C"])
        assert row.limit % Z.GRID_YZ in (0, 1) and row.limit // Z.GRID_YZ in (1, 2)      # z goes 1 -> 2 -> 3 (65,536: the device's)
    if row.quantity == "last_frame_base":
        f, N = row.cross["frame"], row.cross["N"]
        assert (N - 1) * f >= Z.I32 > (N - 2) * f and row.below["N"] == N - 1
        assert N * f * 4 >= Z.U32                                                           # and the tensor is past 2^32 bytes
    assert (row.message is not None) == (row.expect == "refusal")
    assert 0 <= row.peak_bytes < 200 << 30
    if row.expect == "result":
        assert row.peak_bytes > 0
    if row.quantity == "elements" and row.limit == Z.U32:       # a global size is rounded up to whole workgroups of 256
        assert -(-Z.value(row, row.below) // 256) * 256 < Z.U32


def test_depthwise_grid_fold_covers_every_plane():
    """dw_grid of csrc/misc.hip in Python integers: z = ceil(planes / 65535) rows of ceil(planes / z) planes cover every
    plane once, leave fewer than z columns idle, keep y within 65535 and are (1 row, y = planes) up to 65535 planes."""
    for planes in (1, 6, 65534, 65535, 65536, 65537, 131070, 131071, 131075, 70272, 66368, (1 << 31) - 1):
        gz = -(-planes // Z.GRID_YZ)
        gy = -(-planes // gz)
        assert gy <= Z.GRID_YZ and gz <= Z.GRID_YZ
        assert gy * gz >= planes > gy * gz - gz and (gz - 1) * gy < planes
        if planes <= Z.GRID_YZ:
            assert (gy, gz) == (planes, 1)
        assert (gz - 1) * gy + (gy - 1) < Z.U32                 # the kernels form the index unsigned and compare it unsigned


def test_packed_size_queries_equal_their_layouts():
    """The packed-weight queries equal the products of the layouts stated at their declarations, past 2^32 floats too."""
    _, L = _engine()
    lib = L.lib()
    wrapped = 0
    for name, formula in Z.PACKED_FORMULAS.items():
        for cin, coutP in Z.PACKED_SHAPES:
            want = formula(cin, coutP)
            assert getattr(lib, name)(cin, coutP) == want, (name, cin, coutP)
            wrapped += want >= Z.U32
    assert wrapped >= 4                                                                     # the shapes do reach past 32 bits


def test_workspace_queries_equal_their_formulas():
    """Every workspace and size query equals the closed form stated at the end of include/c2s_hip.h, in Python integers, at
    shapes of the rows and at shapes whose result passes 2^32."""
    _, L = _engine()
    lib, F = L.lib(), Z.WORKSPACE_FORMULAS
    past = 0
    for N, C, HW in ((3, 64, 256), (4369, 64, 4096), (65537, 64, 1024), (209717, 32, 2048), (700000, 1024, 65536), (65536, 128, 5000),
                     (2000000, 256, 4096)):
        for kind, groups in ((L.NORM_GROUP, 4), (L.NORM_BATCH, 4), (L.NORM_GROUP, C)):
            nd = L.NormDesc(N, C, HW, kind, groups, 1, 1e-5, 0.1)
            assert lib.c2s_norm_workspace_floats(ctypes.byref(nd)) == F["norm"](N, C, HW), (N, C, HW, kind)
            for has_valid in (0, 1):
                got = lib.c2s_norm_onepass_sync_bytes(ctypes.byref(nd), has_valid)
                assert got in (0, F["norm_onepass_sync"](N, C, HW)), (N, C, HW, kind, has_valid, got)
        assert lib.c2s_se_workspace_floats(N, C, HW) == F["se"](N, C, HW), (N, C, HW)
        assert lib.c2s_pixel_gn_bwd_workspace_floats(N, C, HW) == F["pixel_gn_bwd"](N, C, HW)
        assert lib.c2s_cross_entropy_workspace_floats(N, HW) == F["cross_entropy"](N, HW)
        assert lib.c2s_recall_ce_workspace_floats(N, HW) == F["recall_ce"](N, HW)
        past += F["norm"](N, C, HW) >= Z.U32
    assert past >= 2
    # the one-pass form does take some of these shapes: its formula is not held against 0 alone
    nd = L.NormDesc(8, 64, 4096, L.NORM_GROUP, 4, 1, 1e-5, 0.1)
    assert lib.c2s_norm_onepass_sync_bytes(ctypes.byref(nd), 0) == F["norm_onepass_sync"](8, 64, 4096) > 64
    nd = L.NormDesc(1 << 21, 64, 4096, L.NORM_GROUP, 4, 1, 1e-5, 0.1)               # 2^32 bytes and more
    assert lib.c2s_norm_onepass_sync_bytes(ctypes.byref(nd), 1) == F["norm_onepass_sync"](1 << 21, 64, 4096) > Z.U32
    for nsl, K, cin, cout in ((1, 3, 64, 64), (512, 3, 10, 15), (64, 4, 96, 72), (65537, 6, 1024, 1024), (1 << 20, 3, 1000, 100)):
        d = L.WgradDesc(4, cin, 0, 32, 32, cout, 32, 32, K, K, 1, 1, 1, 0, nsl)
        assert lib.c2s_wgrad_workspace_floats(ctypes.byref(d)) == F["wgrad"](nsl, K, cin, cout), (nsl, K, cin, cout)
    for nh, B, T, H, W in ((16, 2, 9, 32, 32), (16, 18, 61, 16, 16), (16, 262145, 2, 32, 32), (16, 17, 61, 256, 256)):
        d = L.AggDesc(B, T, 64, H, W, nh, H // 4, W // 4)
        assert lib.c2s_temporal_aggregate_bwd_workspace_floats(ctypes.byref(d)) == F["agg_bwd"](nh, B, T, H, W)


def test_workspace_queries_do_not_wrap():
    """The workspace queries whose documentation states no closed form are affine in the frame (or batch) count: the
    second difference over N, 2N, 3N is 0 in Python integers, with 3N frames well past 2^32 floats of workspace where the
    per-frame share allows.  A 32-bit product inside a query breaks that."""
    _, L = _engine()
    lib = L.lib()

    def norm(kind, groups):
        return lambda n: lib.c2s_norm_workspace_floats(ctypes.byref(L.NormDesc(n, 64, 4096, kind, groups, 1, 1e-5, 0.1)))

    def agg(n):
        return lib.c2s_temporal_aggregate_bwd_workspace_floats(ctypes.byref(L.AggDesc(n, 61, 64, 32, 32, 16, 8, 8)))

    def wgrad(n):       # n slices of a 64 -> 64 channel 3x3 layer
        return lib.c2s_wgrad_workspace_floats(ctypes.byref(L.WgradDesc(4, 64, 0, 32, 32, 64, 32, 32, 3, 3, 1, 1, 1, 0, n)))

    queries = {
        "se": lambda n: lib.c2s_se_workspace_floats(n, 1024, 1 << 16),
        "norm-group": norm(L.NORM_GROUP, 4),
        "pixel_gn": lambda n: lib.c2s_pixel_gn_bwd_workspace_floats(n, 128, 1 << 14),
        "cross_entropy": lambda n: lib.c2s_cross_entropy_workspace_floats(n, 1 << 16),
        "recall_ce": lambda n: lib.c2s_recall_ce_workspace_floats(n, 1 << 16),
        "agg_bwd": agg,
        "wgrad": wgrad,
    }
    for name, q in queries.items():
        for n in (1 << 16, 65537, 700000):
            a, b, c = q(n), q(2 * n), q(3 * n)
            assert 0 <= a <= b <= c, (name, n, a, b, c)
            assert c - b == b - a, f"{name}: not affine in the count at {n}: {a}, {b}, {c}"
    n = 700000
    assert queries["se"](3 * n) > Z.U32


@pytest.mark.parametrize("rid,family,export,args", Z.CONV_Z + Z.CONV_WINO, ids=[c[0] for c in Z.CONV_Z + Z.CONV_WINO])
def test_conv_plan_launches_or_refuses(rid, family, export, args, monkeypatch):
    """Across 65,535 / 65,536 / 65,537 (and far above): conv_plan names a family whose launcher takes that N, or raises a
    C2SError that names the limit; it never plans a family that then fails at launch.  Each family's limit in the table is
    held against its launcher: one frame above it the entry point refuses, naming the limit, before any launch."""
    E, L = _engine()
    s = Z._conv_shape(2, *args)
    monkeypatch.setattr(E, "CONV_MODE", s["conv_mode"])
    small = E.conv_plan(*_plan_args(L, s, 2))
    assert small.family == family, (small.family, family)
    for N in (65535, 65536, 65537, 200000):
        try:
            plan = E.conv_plan(*_plan_args(L, s, N))
        except L.C2SError as e:
            assert N > Z.FAMILY_MAX_FRAMES[family] and Z.Z_MESSAGE in str(e), (N, str(e))
            continue
        top = Z.FAMILY_MAX_FRAMES[plan.family]
        assert top is None or N <= top, f"{rid}: N = {N} planned on {plan.family}, whose launcher takes {top} frames"
        assert all(l.desc.N == N for l in plan.launches)
        if N <= Z.FAMILY_MAX_FRAMES[family]:
            assert plan.family == family, f"{rid}: the family changed below its limit ({plan.family} at N = {N})"
    top = Z.FAMILY_MAX_FRAMES[family]
    d = _desc_at(L, small, top + 1)
    if family in ("wino16", "s2wino"):
        pred = {"wino16": L.lib().c2s_conv3x3_winograd16_supported, "s2wino": L.lib().c2s_conv4x4s2_winograd_supported}[family]
        assert pred(ctypes.byref(_desc_at(L, small, top))) == 1 and pred(ctypes.byref(d)) == 0
    if not _no_device():
        return
    assert _launch_unlaunched(L, family, d) == -1
    msg = L.lib().c2s_last_error().decode()
    assert f"more than {top} frames in one launch" in msg, msg
    if family in ("wino16", "s2wino"):
        pred = {"wino16": L.lib().c2s_conv3x3_winograd16_supported, "s2wino": L.lib().c2s_conv4x4s2_winograd_supported}[family]
        assert pred(ctypes.byref(_desc_at(L, small, top))) == 1 and pred(ctypes.byref(d)) == 0


@pytest.mark.parametrize("row", [r for r in Z.ROWS if r.expect == "refusal"], ids=lambda r: r.id)
def test_refusal_rows_refuse_before_any_launch(row, monkeypatch):
    if not _no_device():
        return                                                    # placeholder pointers: see _no_device
    E, L = _engine()
    lib, p = L.lib(), 16
    if "op" in row.cross:
        monkeypatch.setattr(E, "CONV_MODE", row.cross["conv_mode"])
        small = E.conv_plan(*_plan_args(L, row.cross, 2))
        rc = _launch_unlaunched(L, small.family, _desc_at(L, small, row.cross["N"]))
    elif row.export == "c2s_collate_series":
        rc = lib.c2s_collate_series(p, L.SRC_F32, p, None, p, None, None, row.cross["B"], row.cross["T"], 4, 4, 16, None, None,
                                    None, 0.0, None)
    elif row.export in ("c2s_temporal_aggregate_fwd", "c2s_agg_skip_term"):
        c = row.cross
        d = ctypes.byref(L.AggDesc(c["B"], c["T"], c["C"], c["H"], c["W"], c["nh"], c["h"], c["w"]))
        rc = lib.c2s_temporal_aggregate_fwd(d, p, p, None, p, None) if row.export.endswith("fwd") else \
            lib.c2s_agg_skip_term(d, p, p, None, p, None)
    elif row.export == "c2s_pixel_gn_fwd":
        c = row.cross
        rc = lib.c2s_pixel_gn_fwd(p, p, p, p, p, c["B"], c["C"], c["HW"], c["groups"], 1e-5, None)
    else:
        assert row.export == "c2s_ltae_pe_gattn"
        rc = lib.c2s_ltae_pe_gattn(p, p, None, p, row.cross["B"], row.cross["T"], 16, None)
    assert rc == -1 and row.message in lib.c2s_last_error().decode(), lib.c2s_last_error()


def test_depthwise_plane_limits():
    """Forward and data gradient refuse only past 2^31 - 1 planes; the weight gradient, one workgroup of 256 per plane in
    gridDim.x, from 2^24 planes."""
    if not _no_device():
        return
    _, L = _engine()
    lib, p = L.lib(), 16
    assert lib.c2s_dwconv_fwd(p, p, p, None, 65536, 32768, 8, 8, 3, 1, 1, L.PAD_ZEROS, None) == -1
    assert b"2^31 - 1 planes" in lib.c2s_last_error()
    assert lib.c2s_dwconv_dgrad(p, p, p, None, 1 << 20, 1 << 11, 8, 8, 4, 2, 1, L.PAD_ZEROS, 0, None) == -1
    assert b"2^31 - 1 planes" in lib.c2s_last_error()
    assert lib.c2s_dwconv_wgrad(p, p, p, p, None, 1 << 12, 1 << 12, 8, 8, 4, 2, 1, L.PAD_ZEROS, None) == -1
    assert Z.ITEMS_MESSAGE.encode() in lib.c2s_last_error()


def test_one_wave_per_item_launches_refuse_2_32_work_items():
    """The (row, segment) launches of the normalisation and SE kernels run one wave per item: 2^26 items are 2^32
    work-items along gridDim.x.  c2s_frame_flags: N * chunks workgroups of 256."""
    if not _no_device():
        return
    _, L = _engine()
    lib, p = L.lib(), 16
    nd = L.NormDesc(1 << 16, 1 << 10, 16, L.NORM_GROUP, 4, 1, 1e-5, 0.1)             # 2^26 rows of one segment
    assert lib.c2s_norm_fwd(ctypes.byref(nd), p, p, p, None, None, None, p, p, None, p, 1, p, 1 << 40, None, 0.0, None) == -1
    assert Z.ITEMS_MESSAGE.encode() in lib.c2s_last_error()
    assert lib.c2s_se_fwd(p, p, p, p, p, p, p, None, 1 << 16, 1 << 10, 16, 0.0, p, 1 << 40, None) == -1
    assert Z.ITEMS_MESSAGE.encode() in lib.c2s_last_error()
    assert lib.c2s_frame_flags(p, p, 1 << 24, 16, 0.0, None) == -1
    assert Z.ITEMS_MESSAGE.encode() in lib.c2s_last_error()


def test_kernel_choice_does_not_change_across_an_edge():
    """c2s_conv_igemm_split and c2s_wgrad_path give one answer on both sides of 65,535 / 65,536 frames (every launch that
    large fills the device: split 1).  c2s_dwconv_paths takes no count: its answer for the rows' planes is the one the
    per-element table (dw_ref) pins for planes of that kind.  c2s_ltae_paths gives one answer for B * T on both sides of
    65,535 / 65,536 frames, and at the whole-model rows' batch and sub-batch."""
    import dw_ref
    E, L = _engine()
    lib = L.lib()
    want = {(3, 8): (4, 4, 4), (4, 8): (4, 4, 4), (2, 8): (1, 1, 1), (6, 8): (1, 1, 1),
            (3, 6): (1, 1, 1), (4, 6): (1, 1, 1), (2, 6): (1, 1, 1), (6, 6): (1, 1, 1)}
    for K, S, pad, mode, H, W in Z.DW_GEOMS:
        assert dw_ref.paths(L, H, W, K, S, pad, mode) == want[(K, H)], (K, H)
    assert dw_ref.paths(L, 40, 48, 3, 1, 1, "zeros") == (4, 4, 4)

    def ltae(B, T, C, HW):
        d = L.LtaeDesc(B, T, C, HW, 16, 256, 1e-5, 0.1, 0, None, None)
        f, b = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.c2s_ltae_paths(ctypes.byref(d), 1, ctypes.byref(f), ctypes.byref(b)) == 0
        return f.value, b.value

    assert len({ltae(B, 61, 64, 64) for B in (1074, 1075)}) == 1          # B * T = 65,514 and 65,575
    assert len({ltae(B, 64, 64, 64) for B in (1023, 1024, 1025)}) == 1    # 65,472, 65,536, 65,600
    assert ltae(18, 61, 64, 256) == ltae(6, 61, 64, 256)                  # TimeUNet row and its sub-batches
    for rid, family, export, args in Z.CONV_Z:
        if family != "igemm":
            continue
        small = E.conv_plan(*_plan_args(L, Z._conv_shape(2, *args), 2))
        splits = {lib.c2s_conv_igemm_split(ctypes.byref(_desc_at(L, small, N)), 256) for N in (65534, 65535, 65536, 65537)}
        assert splits == {1}, (rid, splits)
    fams = set()
    for N in (65535, 65536, 65537):
        fam = ctypes.c_int(-1)
        d = L.WgradDesc(N, 16, 0, 4, 4, 16, 4, 4, 3, 3, 1, 1, 1, L.PAD_REFLECT, 64)
        assert lib.c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == 0
        fams.add(fam.value)
    assert len(fams) == 1, fams
