"""The kernels past their frame-count and 2^31-element edges (rows: tests/size_rows.py; the host side of the same rows:
tests/test_size_rows.py).

What a row does.  Exports whose frames are independent run the large launch once into an output that is a slice of a larger
allocation, one sentinel frame before it and one after it; on the check frames (the first, the last below the limit, the
first at or above it, the last) the result must equal bit for bit the same export run on those frames alone (same plan:
C2S_IGEMM_SPLIT is forced where the split depends on N), and that small run is held to float64 per element by the family's
existing rule and constant (C_FAMILY, C_OP, the bf16x3 rule, tail_ref's Adam bound).  The sentinel frames must be untouched
and frames with valid == 0 must hold what the export leaves there (the prefill; 0 for a fresh depthwise data gradient).
The depthwise rows at 65,535 - 131,075 planes hold EVERY plane to float64 (8 M elements; torch's grouped convolution on the
CPU takes a second), the weight gradient included: its per-plane partial sums are the ones the small rows pin, and the sum
over the frames runs in double, so C_FAMILY["dw_wgrad"] holds with A summed over all frames.  No tolerance is new here.

The launches with one thread per item (aggregation, per-pixel GroupNorm) run at the largest gridDim.x x blockDim.x the exports take,
just below 2^32 work-items: above it HIP accepts the launch and does not run all of it, and the exports refuse (test_size_rows.py).

A row skips only when the device reports less free memory than its stated peak; on a device of 256 GB or more the last test
fails if any row skipped.  The row's wall time and peak bytes are printed by the last test (profiles/size_limit_times.txt).
"""
import time

import pytest
import torch

import conv_ref as R
import size_rows as Z
import tail_ref as TR
from test_conv_modes_gpu import FROB_BF16X3, U_BF16X3
from test_conv_paths_gpu import C_FAMILY, SENTINEL, _ctx, _gen
from test_size_rows import _plan_args
from test_strided_geometry_gpu import C_OP

pytestmark = pytest.mark.gpu

SKIPPED = []
TIMES = {}              # row id -> (seconds, peak bytes allocated)
STEP_LIMIT_S = 240      # every row runs under its own time limit


@pytest.fixture(autouse=True)
def _time_limit():
    """SIGALRM with its default action: a row that hangs, inside a driver call included, ends the process instead of the
    suite waiting on it (the slowest row takes a few seconds)."""
    import signal
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(STEP_LIMIT_S)
    yield
    signal.alarm(0)


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


class _Row:
    """Skip when the device has less free memory than the row's peak; time the row and record its peak allocation; free the
    row's tensors before the next one."""

    def __init__(self, rid, peak_bytes):
        self.rid, self.peak = rid, peak_bytes

    def __enter__(self):
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free < self.peak:
            SKIPPED.append(self.rid)
            pytest.skip(f"{self.rid}: {free >> 20} MiB free, the row needs {self.peak >> 20} MiB")
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        TIMES[self.rid] = (time.perf_counter() - self.t0, torch.cuda.max_memory_allocated())
        torch.cuda.empty_cache()
        return False


def _bits_equal(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def _framed(shape, fill=SENTINEL):
    """A tensor of `shape` [N, ...] inside an allocation with one sentinel frame on each side: (allocation, view)."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, device="cuda", dtype=torch.float32)
    return buf, buf[1:shape[0] + 1]


def _sentinels_untouched(buf, what):
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), f"{what}: a sentinel frame was written"


def _check_frames(N, limit_frame):
    """First, last below the limit, first at or above it, last (frame indices, deduplicated, in range)."""
    return sorted({f for f in (0, limit_frame - 1, limit_frame, N - 1) if 0 <= f < N})


def _holes(N, frames):
    """Frames with valid == 0: none of the check frames."""
    return sorted({f for f in (1, N // 3, N - 2) if 0 < f < N - 1 and f not in frames})


# ================================================================================================= depthwise, L1
def _fold_frames(N, C):
    """Frames on both sides of every seam of dw_grid (csrc/misc.hip): z = ceil(planes / 65535) grid rows of ceil(planes / z)
    planes each, so row k starts at plane k * gy (at 65,536 planes: 2 rows of 32,768).  At most the first, a middle and the
    last seam when there are many rows."""
    planes = N * C
    gz = -(-planes // Z.GRID_YZ)
    gy = -(-planes // gz)
    seams = sorted({k for k in (1, gz // 2, gz - 1) if 0 < k < gz})
    return sorted({f for k in seams for f in ((k * gy - 1) // C, (k * gy) // C) if 0 <= f < N})


DW_CASES = [(g, planes) for g in Z.DW_GEOMS for planes in (65535, 65536, 65537, 131075)]


def _dw_constants(K):
    return dict(C_OP) if K in (2, 6) else {"fwd": C_FAMILY["dw"], "dgrad": C_FAMILY["dw"], "wgrad": C_FAMILY["dw_wgrad"]}


def _dw_launch(L, x, w, out, gout, gin_fresh, gin_acc, gw, vd, N, C, H, W, K, S, pad, pm):
    """The three exports on device tensors (any of out / gin_fresh / gin_acc / gw may be None)."""
    lib, chk, vp = L.lib(), L.check, (vd.data_ptr() if vd is not None else None)
    if out is not None:
        chk(lib.c2s_dwconv_fwd(x.data_ptr(), w.data_ptr(), out.data_ptr(), vp, N, C, H, W, K, S, pad, pm, None), "dwconv_fwd")
    if gin_fresh is not None:
        chk(lib.c2s_dwconv_dgrad(gout.data_ptr(), w.data_ptr(), gin_fresh.data_ptr(), vp, N, C, H, W, K, S, pad, pm, 0, None),
            "dwconv_dgrad")
    if gin_acc is not None:
        chk(lib.c2s_dwconv_dgrad(gout.data_ptr(), w.data_ptr(), gin_acc.data_ptr(), vp, N, C, H, W, K, S, pad, pm, 1, None),
            "dwconv_dgrad")
    if gw is not None:
        part = torch.empty(N * C * K * K, device="cuda")
        chk(lib.c2s_dwconv_wgrad(x.data_ptr(), gout.data_ptr(), part.data_ptr(), gw.data_ptr(), vp, N, C, H, W, K, S, pad, pm,
                                 None), "dwconv_wgrad")


@pytest.mark.parametrize("geom,planes", DW_CASES, ids=[f"k{g[0]}-{g[4]}x{g[5]}-{p}" for g, p in DW_CASES])
def test_depthwise_planes(geom, planes):
    _, L = _engine()
    K, S, pad, mode, H, W = geom
    N, C = Z.DW_COUNTS[planes]
    Ho, Wo = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    pm = L.PAD_REFLECT if mode == "reflect" else L.PAD_ZEROS
    rid = f"dw-k{K}-{H}x{W}-{planes}"
    shape = dict(N=N, C=C, K=K, S=S, pad=pad, mode=mode, H=H, W=W)
    with _Row(rid, Z._dw_bytes(shape)):
        g = _gen(rid)
        frames = sorted(set(_check_frames(N, Z.GRID_YZ // C)) | set(_fold_frames(N, C)))     # plane 65,535; the grid rows' seams
        keep = torch.ones(N, dtype=torch.bool)
        keep[_holes(N, frames)] = False
        x, gout = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, Ho, Wo, generator=g)
        w, prior = torch.randn(C, 1, K, K, generator=g), torch.randn(N, C, H, W, generator=g)
        x[~keep], gout[~keep], prior[~keep] = float("nan"), float("nan"), SENTINEL
        xd, gd, wd, vd = x.cuda(), gout.cuda(), w.cuda(), keep.int().cuda()
        obuf, out = _framed((N, C, Ho, Wo))
        fbuf, fresh = _framed((N, C, H, W))
        abuf, acc = _framed((N, C, H, W))
        acc.copy_(prior)
        gw = torch.full((C, 1, K, K), float("nan"), device="cuda")
        _dw_launch(L, xd, wd, out, gd, fresh, acc, gw, vd, N, C, H, W, K, S, pad, pm)
        torch.cuda.synchronize()
        for buf, what in ((obuf, "forward"), (fbuf, "data gradient"), (abuf, "accumulated data gradient")):
            _sentinels_untouched(buf, f"{rid} {what}")
        got_y, got_f, got_a = out.cpu(), fresh.cpu(), acc.cpu()
        assert bool((got_y[~keep] == SENTINEL).all()), f"{rid}: the forward wrote a frame with valid == 0"
        assert bool((got_f[~keep] == 0).all()), f"{rid}: a fresh data gradient is not 0 on the frames with valid == 0"
        assert _bits_equal(got_a[~keep], prior[~keep]), f"{rid}: an accumulated data gradient changed a frame with valid == 0"

        # the check frames alone: the same bits
        idx = torch.tensor(frames)
        n = len(frames)
        so = torch.full((n, C, Ho, Wo), SENTINEL, device="cuda")
        sf = torch.full((n, C, H, W), SENTINEL, device="cuda")
        _dw_launch(L, x[idx].cuda(), wd, so, gout[idx].cuda(), sf, None, None, None, n, C, H, W, K, S, pad, pm)
        torch.cuda.synchronize()
        assert _bits_equal(got_y[idx], so.cpu()), f"{rid}: forward bits of frames {frames} depend on the launch"
        assert _bits_equal(got_f[idx], sf.cpu()), f"{rid}: data-gradient bits of frames {frames} depend on the launch"

        # every plane against float64
        c = _dw_constants(K)
        ref = R.conv_refs(x[keep], w, None, gout[keep], S, pad, mode, groups=C)
        p64 = prior[keep].double()
        ratios = (R.assert_within(f"{rid} forward", got_y[keep], ref["y"], ref["Ay"], c["fwd"], R.FROB_FWD),
                  R.assert_within(f"{rid} data gradient", got_f[keep], ref["gx"], ref["Agx"], c["dgrad"], R.FROB_GRAD),
                  R.assert_within(f"{rid} accumulated data gradient", got_a[keep], ref["gx"] + p64, ref["Agx"] + p64.abs(),
                                  c["dgrad"], R.FROB_GRAD),
                  R.assert_within(f"{rid} weight gradient", gw.cpu(), ref["gw"], ref["Agw"], c["wgrad"], R.FROB_GRAD))
        print(f"\n{rid}: N {N} x C {C}, check frames {frames}: " + "  ".join(f"{r:.2f}" for r in ratios))


# ================================================================================================= convolutions, L1
CONV_CASES = [(c, 65535) for c in Z.CONV_Z] + [(c, 65536) for c in Z.CONV_WINO]


def _conv_rule(family):
    if family == "bf16x3":
        return U_BF16X3 / R.U + C_FAMILY["igemm"], FROB_BF16X3, FROB_BF16X3
    if family == "smallcin":                            # test_conv_modes_gpu.BOUNDS: the first-layer kernel at the igemm constant
        return C_FAMILY["igemm"], R.FROB_FWD, R.FROB_GRAD
    return C_FAMILY[family], R.FROB_FWD, R.FROB_GRAD


@pytest.mark.parametrize("case,N", CONV_CASES, ids=[f"{c[0]}-{n}" for c, n in CONV_CASES])
def test_conv_frames(case, N, monkeypatch):
    """The largest frame count each family takes: 65,535 for the gridDim.z families, 65,536 for the 8-wave Winograd ones."""
    rid, family, export, args = case
    assert N == Z.FAMILY_MAX_FRAMES[family]
    _conv_case(f"{rid}-{N}", family, args, N, _check_frames(N, min(N - 1, Z.GRID_YZ)), monkeypatch, {})


@pytest.mark.parametrize("case", Z.CONV_L2, ids=[c[0] for c in Z.CONV_L2])
def test_conv_frames_past_2_31(case, monkeypatch):
    """Every conv family with the last frame's base at or above 2^31 elements on its smaller side: frames on both sides of
    2^30 and 2^31 elements (2^32 and 2^33 bytes) of the input and of the output, where the 32-bit per-frame byte offsets meet
    the 64-bit frame base."""
    rid, family, export, args, switches = case
    N, frames = Z.conv_l2_frames(args)
    src, dst = Z.conv_frames(Z._conv_shape(N, *args))
    assert (N - 1) * min(src, dst) >= Z.I32
    _conv_case(rid, family, args, N, frames, monkeypatch, switches)


def _conv_case(rid, family, args, N, frames, monkeypatch, switches):
    E, L = _engine()
    s = Z._conv_shape(N, *args)
    monkeypatch.setattr(E, "CONV_MODE", s["conv_mode"])
    for name, value in switches.items():                # the engine switches that put the shape on the family
        monkeypatch.setattr(E, name, value)
    monkeypatch.setenv("C2S_IGEMM_SPLIT", "1")          # the split of the small run is the large run's
    op, K, S, pad, mode = s["op"], s["K"], s["S"], s["pad"], s["mode"]
    Cin, Cout, H, W = sum(s["chans"]), s["Cout"], s["H"], s["W"]
    Ho, Wo = Z.conv_out_hw(s)
    src_f, dst_f = Z.conv_frames(s)
    with _Row(rid, 4 * (N * src_f + (N + 2) * dst_f + N) + (1 << 30)):
        plan = E.conv_plan(*_plan_args(L, s, N))
        assert plan.family == family, plan.family
        gen = _gen(f"size-{rid}")
        w = torch.randn((Cin, Cout, K, K) if op == "tfwd" else (Cout, Cin, K, K), generator=gen) / (Cin * K * K) ** 0.5
        b = torch.randn(Cout, generator=gen)
        ctx = _ctx({"w": w, "b": b})
        dg = torch.Generator(device="cuda").manual_seed(int(gen.initial_seed()))
        src_shape, out_shape = ((N, Cout, Ho, Wo), (N, Cin, H, W)) if op == "dgrad" else ((N, Cin, H, W), (N, Cout, Ho, Wo))
        holes = [] if op == "tfwd" else _holes(N, frames)      # the transposed forward takes no frame flags in the engine
        src = torch.empty(src_shape, device="cuda")
        for lo, hi in _chunks(N, max(1, (1 << 28) // src_f)):
            src[lo:hi].normal_(generator=dg)
        keep = torch.ones(N, dtype=torch.bool)
        keep[holes] = False
        src[torch.tensor(holes, dtype=torch.long)] = float("nan")
        vd = None if op == "tfwd" else keep.int().cuda()
        bias = None if op == "dgrad" else ctx.p["b"]
        obuf, out = _framed(out_shape)
        E._run_conv(ctx, plan, "w", ctx.p["w"], src, None, bias, out, vd)
        torch.cuda.synchronize()
        _sentinels_untouched(obuf, rid)
        if holes:
            assert bool((out[torch.tensor(holes)] == SENTINEL).all()), f"{rid}: a frame with valid == 0 was written"

        idx = torch.tensor(frames, device="cuda")
        small_plan = E.conv_plan(*_plan_args(L, s, len(frames)))
        assert small_plan.family == family, (small_plan.family, family)
        ssrc = src[idx].contiguous()
        sout = torch.full((len(frames),) + tuple(out_shape[1:]), SENTINEL, device="cuda")
        E._run_conv(ctx, small_plan, "w", ctx.p["w"], ssrc, None, bias, sout, None)
        torch.cuda.synchronize()
        assert _bits_equal(out[idx], sout), f"{rid}: bits of frames {frames} depend on the launch they are in"

        c, frob_f, frob_g = _conv_rule(family)
        xs, got = ssrc.cpu(), sout.cpu()
        if op == "dgrad":
            ref = R.conv_refs(torch.zeros((len(frames),) + tuple(out_shape[1:])), w, None, xs, S, pad, mode)
            ratio = R.assert_within(f"{rid} data gradient", got, ref["gx"], ref["Agx"], c, frob_g)
        else:
            ref = R.conv_refs(xs, w, b, torch.zeros((len(frames),) + tuple(out_shape[1:])), S, pad, mode,
                              transpose=op == "tfwd")
            ratio = R.assert_within(f"{rid} forward", got, ref["y"], ref["Ay"], c, frob_f)
        print(f"\n{rid}: N {N} on {family}, check frames {frames}: {ratio:.2f}")


@pytest.mark.parametrize("case", Z.CONV_Z + Z.CONV_WINO, ids=[c[0] for c in Z.CONV_Z + Z.CONV_WINO])
def test_conv_plan_refuses_on_the_device_too(case, monkeypatch):
    """With a device present (its CU count enters the plan) conv_plan still refuses above each family's limit or moves to a
    family that takes the count."""
    E, L = _engine()
    rid, family, export, args = case
    monkeypatch.setattr(E, "CONV_MODE", Z._conv_shape(2, *args)["conv_mode"])
    for N in (Z.FAMILY_MAX_FRAMES[family] + 1, 65537):
        try:
            plan = E.conv_plan(*_plan_args(L, Z._conv_shape(N, *args), N))
        except L.C2SError as e:
            assert Z.Z_MESSAGE in str(e)
            continue
        top = Z.FAMILY_MAX_FRAMES[plan.family]
        assert top is None or N <= top, (rid, N, plan.family)


# ================================================================================================= cut_windows, L1
CUT_SHAPES = [Z.BY_ID["cut-windows-65536"].below, Z.BY_ID["cut-windows-65536"].cross, Z.BY_ID["cut-windows-65537"].cross]


@pytest.mark.parametrize("s", CUT_SHAPES, ids=[f"frames-{s['N']}" for s in CUT_SHAPES])
def test_cut_windows_frames(s):
    """65,535 / 65,536 / 65,537 output frames: the launch clamps gridDim.z at 65,535 and loops.  A copy: every element of
    every window equals the raster's, the origins being those of raster_ref.window_origins."""
    import raster_ref
    _, L = _engine()
    T, C, H, W, ph, pw, first, nwin = (s[k] for k in ("T", "C", "H", "W", "ph", "pw", "first", "nwin"))
    frames = nwin * T
    assert frames == s["N"]
    with _Row(f"cut-windows-{frames}", 4 * ((frames + 2) * C * ph * pw * 2 + T * C * H * W)):
        series = torch.randn(T, C, H, W, generator=_gen(f"cut-{frames}"))
        assert raster_ref.window_origins(H, ph, 1) == list(range(H - ph + 1))          # stride 1, exact fit: origin i
        assert raster_ref.window_origins(W, pw, 1) == list(range(W - pw + 1))
        sd = series.cuda()
        xbuf, x = _framed((frames, C, ph, pw))
        L.check(L.lib().c2s_cut_windows(sd.data_ptr(), x.data_ptr(), T, C, H, W, ph, pw, 1, 1, first, nwin, 0, None, None),
                "cut_windows")
        torch.cuda.synchronize()
        _sentinels_untouched(xbuf, f"cut-windows-{frames}")
        # [T, C, ny, nx, ph, pw] -> [window, T, C, ph, pw], windows row-major
        want = sd.unfold(2, ph, 1).unfold(3, pw, 1).permute(2, 3, 0, 1, 4, 5).reshape(-1, T, C, ph, pw)[first:first + nwin]
        assert _bits_equal(x.view(nwin, T, C, ph, pw), want.contiguous())


# ================================================================================================= flat buffers, L2
def _chunks(n, step=1 << 28):
    return [(lo, min(n, lo + step)) for lo in range(0, n, step)]


def test_fill_past_2_31():
    _, L = _engine()
    row = Z.BY_ID["fill-2^31"]
    n = row.cross["n"]
    with _Row(row.id, row.peak_bytes + (1 << 30)):
        buf = torch.full((n + 2,), SENTINEL, device="cuda")
        L.check(L.lib().c2s_fill(buf[1:].data_ptr(), n, 3.25, None), "fill")
        torch.cuda.synchronize()
        assert float(buf[0]) == SENTINEL and float(buf[n + 1]) == SENTINEL
        for lo, hi in _chunks(n):
            assert bool((buf[1 + lo:1 + hi] == 3.25).all()), f"fill: elements {lo} .. {hi} not all written"


def test_add_inplace_past_2_31():
    """Every element: the float32 sum is correctly rounded, so torch's own add gives the bits."""
    _, L = _engine()
    row = Z.BY_ID["add-2^31"]
    n = row.cross["n"]
    with _Row(row.id, row.peak_bytes + 4 * n + 3 * (1 << 30)):
        dg = torch.Generator(device="cuda").manual_seed(31)
        dbuf = torch.full((n + 2,), SENTINEL, device="cuda")
        d = dbuf[1:n + 1]
        s = torch.empty(n, device="cuda")
        for lo, hi in _chunks(n):
            d[lo:hi].normal_(generator=dg)
            s[lo:hi].normal_(generator=dg)
        d0 = d.clone()
        L.check(L.lib().c2s_add_inplace(d.data_ptr(), s.data_ptr(), n, None), "add_inplace")
        torch.cuda.synchronize()
        assert float(dbuf[0]) == SENTINEL and float(dbuf[n + 1]) == SENTINEL
        for lo, hi in _chunks(n):
            assert _bits_equal(d[lo:hi], d0[lo:hi] + s[lo:hi]), f"add: wrong in elements {lo} .. {hi}"


def test_adam_flat_past_2_31():
    """Adam is elementwise: windows at the head, around element 2^31 and at the tail equal bit for bit the same export on
    those elements alone, and that small run meets tail_ref's float64 bound (test_tail_reference_gpu.test_adam)."""
    E, L = _engine()
    row = Z.BY_ID["adam-2^31"]
    n = row.cross["n"]
    with _Row(row.id, row.peak_bytes + (1 << 30)):
        dg = torch.Generator(device="cuda").manual_seed(32)
        pbuf = torch.full((n + 2,), SENTINEL, device="cuda")
        p = pbuf[1:n + 1]
        g, m, v = (torch.empty(n, device="cuda") for _ in range(3))
        for lo, hi in _chunks(n):
            p[lo:hi].normal_(generator=dg)
            g[lo:hi].normal_(generator=dg)
            m[lo:hi].normal_(generator=dg).mul_(0.1)
            v[lo:hi].uniform_(0.0, 0.01, generator=dg)
        windows = [(0, 4096), (Z.I32 - 4096, Z.I32 + 5), (n - 4096, n)]
        before = [tuple(t[lo:hi].clone() for t in (p, g, m, v)) for lo, hi in windows]
        step = 1000                                     # bc2 = 0.63: the tight check of the step size (tail_ref.adam_upd_frob)
        E.adam_flat(p, g, m, v, step)
        torch.cuda.synchronize()
        assert float(pbuf[0]) == SENTINEL and float(pbuf[n + 1]) == SENTINEL
        for (lo, hi), (p0, g0, m0, v0) in zip(windows, before):
            ps, ms, vs = p0.clone(), m0.clone(), v0.clone()
            E.adam_flat(ps, g0, ms, vs, step)
            torch.cuda.synchronize()
            for name, large, small in (("p", p, ps), ("m", m, ms), ("v", v, vs)):
                assert _bits_equal(large[lo:hi], small), f"adam: {name} of elements {lo} .. {hi} depends on the launch"
            assert _bits_equal(g[lo:hi], g0)
            ref, A = TR.adam_ref(p0.cpu(), g0.cpu(), m0.cpu(), v0.cpu(), step)
            for name, got in (("m", ms), ("v", vs), ("p", ps)):
                TR.assert_within(f"adam {name} {lo}", got.double().cpu(), ref[name], A[name], TR.C_BOUND, TR.ADAM_FROB)
            upd = ps.double().cpu() - p0.double().cpu()
            TR.assert_within(f"adam upd {lo}", upd, ref["upd"], A["upd"], TR.C_BOUND, TR.adam_upd_frob(ref, A))


# ================================================================================================= frames past 2^31, L2
def test_depthwise_frames_past_2_31():
    """dw_ref's k3-zeros plane (6 channels of 40 x 48, two blocks per plane of the 4-pixel kernels) with the last frame's base
    at or above 2^31 elements: 1.1 M planes, 18 rows of the folded grid."""
    _, L = _engine()
    row = Z.BY_ID["dw-k3-40x48-2^31"]
    s = row.cross
    N, C, H, W, K, S, pad = s["N"], s["C"], s["H"], s["W"], s["K"], s["S"], s["pad"]
    with _Row(row.id, row.peak_bytes):
        dg = torch.Generator(device="cuda").manual_seed(33)
        # the last frame is the one whose base crosses; and the frames at the first, a middle and the last seam of the 18 grid rows
        frames = sorted(set(_check_frames(N, N - 1)) | set(_fold_frames(N, C)))
        keep = torch.ones(N, dtype=torch.bool)
        keep[_holes(N, frames)] = False
        vd = keep.int().cuda()
        x = torch.empty(N, C, H, W, device="cuda")
        for lo, hi in _chunks(N, 1 << 14):
            x[lo:hi].normal_(generator=dg)
        w = torch.randn(C, 1, K, K, generator=_gen(row.id))
        wd = w.cuda()
        obuf, out = _framed((N, C, H, W))
        _dw_launch(L, x, wd, out, None, None, None, None, vd, N, C, H, W, K, S, pad, L.PAD_ZEROS)
        torch.cuda.synchronize()
        _sentinels_untouched(obuf, row.id)
        hole = torch.nonzero(~keep).flatten()
        assert bool((out[hole] == SENTINEL).all())
        idx = torch.tensor(frames, device="cuda")
        xs = x[idx].contiguous()
        so = torch.full((len(frames), C, H, W), SENTINEL, device="cuda")
        _dw_launch(L, xs, wd, so, None, None, None, None, None, len(frames), C, H, W, K, S, pad, L.PAD_ZEROS)
        torch.cuda.synchronize()
        assert _bits_equal(out[idx], so), f"{row.id}: forward bits of frames {frames} depend on the launch"
        # the data gradient of the same launch: `out` of the forward is its gout (same plane size for 3x3 / stride 1), x its
        # destination -- reusing both keeps the row at two large tensors
        gs = out[idx].contiguous()
        _dw_launch(L, None, wd, None, out, x, None, None, vd, N, C, H, W, K, S, pad, L.PAD_ZEROS)
        sg = torch.full((len(frames), C, H, W), SENTINEL, device="cuda")
        _dw_launch(L, None, wd, None, gs, sg, None, None, None, len(frames), C, H, W, K, S, pad, L.PAD_ZEROS)
        torch.cuda.synchronize()
        assert _bits_equal(x[idx], sg), f"{row.id}: data-gradient bits of frames {frames} depend on the launch"
        assert bool((x[hole] == 0).all())
        ref = R.conv_refs(xs.cpu(), w, None, gs.cpu(), S, pad, "zeros", groups=C)
        R.assert_within(f"{row.id} forward", so.cpu(), ref["y"], ref["Ay"], C_FAMILY["dw"], R.FROB_FWD)
        R.assert_within(f"{row.id} data gradient", sg.cpu(), ref["gx"], ref["Agx"], C_FAMILY["dw"], R.FROB_GRAD)
        # the weight gradient sums over the frames: zeros everywhere but a handful of frames on both sides of the edge (zeros
        # are exact in every order of summation), against float64 of those frames alone, A over them
        sel = sorted({0, 5, N // 2, N - 2, N - 1})
        g2 = _gen(row.id + "-wgrad")
        x2, go2 = torch.randn(len(sel), C, H, W, generator=g2), torch.randn(len(sel), C, H, W, generator=g2)
        x.zero_()
        out.zero_()
        x[sel], out[sel] = x2.cuda(), go2.cuda()
        gw = torch.full((C, 1, K, K), float("nan"), device="cuda")
        _dw_launch(L, x, wd, None, out, None, None, gw, None, N, C, H, W, K, S, pad, L.PAD_ZEROS)
        torch.cuda.synchronize()
        ref = R.conv_refs(x2, w, None, go2, S, pad, "zeros", groups=C)
        R.assert_within(f"{row.id} weight gradient", gw.cpu(), ref["gw"], ref["Agw"], C_FAMILY["dw_wgrad"], R.FROB_GRAD)


def test_channel_bias_add_past_2_31():
    """x[n, c, :] += bias[c] on the real frames, in place, every element: a float32 add is correctly rounded, so torch's own
    add gives the bits."""
    _, L = _engine()
    row = Z.BY_ID["bias-add-2^31"]
    N, C, HW = row.cross["N"], row.cross["C"], row.cross["HW"]
    with _Row(row.id, 2 * row.peak_bytes):
        dg = torch.Generator(device="cuda").manual_seed(34)
        frames = _check_frames(N, N - 1)
        keep = torch.ones(N, dtype=torch.bool)
        keep[_holes(N, frames)] = False
        kd = keep.cuda()
        xbuf, x = _framed((N, C, HW))
        for lo, hi in _chunks(N, 1 << 14):
            x[lo:hi].normal_(generator=dg)
        x0 = x.clone()
        bias = torch.randn(C, generator=_gen(row.id)).cuda()
        L.check(L.lib().c2s_channel_bias_add(x.data_ptr(), bias.data_ptr(), kd.int().data_ptr(), N, C, HW, None), "bias_add")
        torch.cuda.synchronize()
        _sentinels_untouched(xbuf, row.id)
        for lo, hi in _chunks(N, 1 << 14):
            want = torch.where(kd[lo:hi].view(-1, 1, 1), x0[lo:hi] + bias.view(1, C, 1), x0[lo:hi])
            assert _bits_equal(x[lo:hi], want), f"{row.id}: wrong in frames {lo} .. {hi}"


def test_frame_flags_past_2_31():
    """valid[n] = any(x[n] != pad_value) with one differing value in a few frames on both sides of the edge: every flag."""
    _, L = _engine()
    row = Z.BY_ID["frame-flags-2^31"]
    N, fe = row.cross["N"], row.cross["frame_elems"]
    with _Row(row.id, row.peak_bytes + (1 << 28)):
        x = torch.full((N, fe), -1.0, device="cuda")
        real = {0: 0, 5: fe - 1, N // 2: 300, N - 3: fe - 1, N - 2: 0, N - 1: fe - 1}      # frame -> the one real position
        for f, pos in real.items():
            x[f, pos] = 0.5
        valid = torch.full((N + 2,), 7, device="cuda", dtype=torch.int32)
        L.check(L.lib().c2s_frame_flags(x.data_ptr(), valid[1:].data_ptr(), N, fe, -1.0, None), "frame_flags")
        torch.cuda.synchronize()
        assert int(valid[0]) == 7 and int(valid[N + 1]) == 7
        want = torch.zeros(N, dtype=torch.int32)
        want[list(real)] = 1
        assert torch.equal(valid[1:N + 1].cpu(), want)


# ================================================================================================= 2^32 work-items, L3
def test_aggregate_fwd_below_2_32_work_items():
    """One thread per (sample, head, pixel): 2^32 - 16,384 of them, the largest launch the export takes (at 2^32 + 16,384 HIP
    accepted the launch and the last sample was never written: the export refuses that now, test_size_rows.py).  The first
    and the last samples equal the same export on those samples alone, which meets norm_ref.agg_ref."""
    import ctypes
    import norm_ref as NR
    _, L = _engine()
    row = Z.BY_ID["agg-fwd-2^32"]
    s = row.below
    B, T, C, H, W, nh, h, w = (s[k] for k in ("B", "T", "C", "H", "W", "nh", "h", "w"))
    with _Row(row.id, row.peak_bytes + (2 << 30)):
        dg = torch.Generator(device="cuda").manual_seed(35)
        x = torch.empty(B, T, C, H, W, device="cuda")
        for lo, hi in _chunks(B, 1 << 13):
            x[lo:hi].normal_(generator=dg)
        attn = torch.rand(nh, B, T, h, w, device="cuda", generator=dg)
        b_lim = B - 1                                   # the last sample ends 16,384 work-items below 2^32
        samples = _check_frames(B, b_lim)
        keep = torch.ones(B, T, dtype=torch.bool)
        for b in _holes(B, samples) + samples[-1:]:
            keep[b, 1] = False                           # a padded second frame, also in the last sample
        x[~keep.cuda()] = float("nan")
        vd = keep.view(-1).int().cuda()
        obuf, out = _framed((B, C, H, W))
        fwd = L.lib().c2s_temporal_aggregate_fwd
        L.check(fwd(ctypes.byref(L.AggDesc(B, T, C, H, W, nh, h, w)), x.data_ptr(), attn.data_ptr(), vd.data_ptr(),
                    out.data_ptr(), None), "temporal_aggregate_fwd")
        torch.cuda.synchronize()
        _sentinels_untouched(obuf, row.id)
        idx = torch.tensor(samples, device="cuda")
        xs, ats, ks = x[idx].contiguous(), attn[:, idx].contiguous(), keep[idx.cpu()]
        so = torch.full((len(samples), C, H, W), SENTINEL, device="cuda")
        L.check(fwd(ctypes.byref(L.AggDesc(len(samples), T, C, H, W, nh, h, w)), xs.data_ptr(), ats.data_ptr(),
                    ks.view(-1).int().cuda().data_ptr(), so.data_ptr(), None), "temporal_aggregate_fwd")
        torch.cuda.synchronize()
        assert _bits_equal(out[idx], so), f"{row.id}: bits of samples {samples} depend on the launch"
        o, A = NR.agg_ref(xs.cpu(), ats.cpu(), ks)
        NR.assert_within(row.id, so.cpu(), o["out"], A["out"], NR.C_BOUND, NR.FROB["out"])


def test_pixel_gn_fwd_below_2_32_work_items():
    """One thread per (sample, group, pixel): 2^32 - 65,536 of them, the largest launch the export takes; the first and the
    last samples against the same export on those samples alone, which meets norm_ref.pixel_gn_ref."""
    import norm_ref as NR
    _, L = _engine()
    row = Z.BY_ID["pixel-gn-fwd-2^32"]
    s = row.below
    B, C, HW, groups = s["B"], s["C"], s["HW"], s["groups"]
    with _Row(row.id, row.peak_bytes + (2 << 30)):
        dg = torch.Generator(device="cuda").manual_seed(36)
        x = torch.empty(B, C, HW, device="cuda")
        for lo, hi in _chunks(B, 1 << 11):
            x[lo:hi].normal_(generator=dg)
        g = _gen(row.id)
        gamma, beta = (torch.randn(C, generator=g) * 0.5 + 1).cuda(), torch.randn(C, generator=g).cuda()
        ybuf, y = _framed((B, C, HW))
        stats = torch.empty(B * groups * HW * 2, device="cuda")
        fwd = L.lib().c2s_pixel_gn_fwd
        L.check(fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), stats.data_ptr(), B, C, HW, groups, 1e-5,
                    None), "pixel_gn_fwd")
        torch.cuda.synchronize()
        _sentinels_untouched(ybuf, row.id)
        samples = _check_frames(B, B - 1)
        idx = torch.tensor(samples, device="cuda")
        xs = x[idx].contiguous()
        sy = torch.full((len(samples), C, HW), SENTINEL, device="cuda")
        sst = torch.empty(len(samples) * groups * HW * 2, device="cuda")
        L.check(fwd(xs.data_ptr(), gamma.data_ptr(), beta.data_ptr(), sy.data_ptr(), sst.data_ptr(), len(samples), C, HW,
                    groups, 1e-5, None), "pixel_gn_fwd")
        torch.cuda.synchronize()
        assert _bits_equal(y[idx], sy), f"{row.id}: bits of samples {samples} depend on the launch"
        per = groups * HW * 2
        for k, b in enumerate(samples):
            assert _bits_equal(stats[b * per:(b + 1) * per], sst[k * per:(k + 1) * per]), f"{row.id}: statistics of sample {b}"
        o, A = NR.pixel_gn_ref(xs.cpu(), None, 0.0, gamma.cpu(), beta.cpu(), groups)
        NR.assert_within(row.id, sy.cpu(), o["y"], A["y"], NR.C_BOUND, NR.FROB["pgn_y"])


# ================================================================================================= whole models
def _timeunet():
    from test_configs_gpu import _model
    return _model("timeunet", "tame")


def _wtae():
    from test_configs_gpu import _model
    return _model("wtae", "tame")


def _utae_mbconv():
    import crop2seg_amd as C2S
    from oracle import seeded
    torch.manual_seed(1)
    net = C2S.UTAE(input_dim=10, out_conv=[32, 20], use_mbconv=True)       # MBConv's GroupNorm(4) head: classes % 4 == 0
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 41, "tame"))
    return net.cuda()


# id, model, B, T, H, classes, the depthwise planes of its widest folded layer (frames x channels), samples per sub-batch
MODEL_ROWS = [
    # W-TAE's spatial_reduction is always depthwise-separable (functional.wtae_forward) and runs on the folded B * T frames:
    # 1,098 frames x 64 channels in its first block
    ("wtae-b18-t61-16", _wtae, 18, 61, 16, 15, 18 * 61 * 64, 6),
    # TimeUNet at the same size has no depthwise layer in its default configuration (observed: c2s_dwconv_fwd is never called);
    # the row keeps the 1,098 folded frames of its other kernels against the sub-batches
    ("timeunet-b18-t61-16", _timeunet, 18, 61, 16, 15, None, 6),
    ("utae-mbconv-b4-t33-32", _utae_mbconv, 4, 33, 32, 20, 4 * 33 * 128 * 4, 2),  # the 128-channel stage expanded x 4
]


@pytest.mark.parametrize("rid,build,B,T,H,K,planes,sub", MODEL_ROWS, ids=[m[0] for m in MODEL_ROWS])
def test_model_past_65536_depthwise_planes(rid, build, B, T, H, K, planes, sub, monkeypatch):
    """Eval mode, irregular series lengths: the logits of the full batch equal bit for bit those of the same model on
    sub-batches (six samples for TimeUNet's 18, two for U-TAE's 4), and the parameter gradients of the full batch are the sum of the sub-batches'
    within the eval-mode rule of test_configs_gpu.test_full_size_winograd_vs_direct (flat gradient 1e-3, every tensor above
    1e-3 of the largest 5e-3).  The modules deliver no input gradient, so none is compared."""
    from crop2seg_amd.learning.synthetic import synthetic_batch
    _, L = _engine()
    seen = []
    real = L.lib().c2s_dwconv_fwd

    def spy(x, w, out, valid, N, C, *rest):
        seen.append(N * C)
        return real(x, w, out, valid, N, C, *rest)

    monkeypatch.setattr(L.lib(), "c2s_dwconv_fwd", spy)
    assert planes is None or planes > 65536
    with _Row(rid, 4 << 30):                             # measured: 0.6 and 2.3 GiB
        x, dates, _, lengths = synthetic_batch(B, T, H, H, 1, "cuda", irregular=True)
        assert max(lengths) == T and min(lengths) < T
        net = build().eval()
        gout = torch.randn(B, K, H, H, generator=_gen(rid)).cuda()

        def run(lo, hi):
            net.zero_grad(set_to_none=True)
            logits = net(x[lo:hi].contiguous(), batch_positions=dates[lo:hi].contiguous())
            logits.backward(gout[lo:hi].contiguous())
            torch.cuda.synchronize()
            return logits.detach().clone(), {n: p.grad.detach().double().clone() for n, p in net.named_parameters()}

        full_logits, full_g = run(0, B)
        if planes is None:
            assert not seen, f"{rid}: c2s_dwconv_fwd ran on {sorted(set(seen))} planes, the row says the model has no such layer"
        else:
            assert planes in seen and max(seen) > 65536, f"{rid}: c2s_dwconv_fwd saw {sorted(set(seen))} planes, the row says {planes}"
        assert bool(torch.isfinite(full_logits).all())
        parts = {n: torch.zeros_like(g) for n, g in full_g.items()}
        assert planes is None or planes * sub // B < 65536     # a sub-batch stays below the edge
        for lo in range(0, B, sub):
            hi = min(B, lo + sub)
            logits, g = run(lo, hi)
            assert _bits_equal(full_logits[lo:hi], logits), f"{rid}: logits of samples {lo} .. {hi - 1} depend on the batch"
            for n in g:
                parts[n] += g[n]
        flat = lambda d: torch.cat([d[n].flatten() for n in sorted(d)])
        flat_rel = float((flat(full_g) - flat(parts)).norm() / flat(parts).norm())
        gmax = max(float(g.norm()) for g in parts.values())
        worst = max((float((full_g[n] - parts[n]).norm()) / float(parts[n].norm()), n) for n in parts
                    if float(parts[n].norm()) > 1e-3 * gmax)
        print(f"\n{rid}: depthwise planes seen {sorted(set(seen))}; gradients full vs sub-batches: flat {flat_rel:.1e}, worst {worst[0]:.1e} ({worst[1]})")
        assert flat_rel <= 1e-3 and worst[0] <= 5e-3, (flat_rel, worst)


# ================================================================================================= the record
def test_no_row_skipped_on_a_large_device():
    total = torch.cuda.mem_get_info()[1]
    print(f"\ndevice memory {total >> 30} GiB; rows: seconds, peak MiB allocated")
    for rid, (sec, peak) in TIMES.items():
        print(f"    {rid:32s} {sec:7.2f} s {peak >> 20:8d} MiB")
    if total >= 256 << 30:
        assert not SKIPPED, f"rows skipped on a device of {total >> 30} GiB: {SKIPPED}"
