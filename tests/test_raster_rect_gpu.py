"""Rectangular patches and unequal strides of sliding-window inference on the GPU.

predict_raster and window_frames take patch=(ph, pw) and stride=(sy, sx), and every entry point of the library takes the
four integers separately, but test_raster_gpu.py and test_raster_raw_gpu.py pass one scalar for each throughout: a swapped
ph / pw or sy / sx in c2s_cut_windows, c2s_cut_windows_raw, c2s_window_frames, c2s_softmax_blend, or in how inference.py
hands them on, would pass both files.  Here the same checks run with patch (16, 32) at stride (12, 24) and patch (32, 16)
at stride (24, 12), on rasters of 40 x 75 and 75 x 40 and on rasters smaller than the window on one axis only (12 x 50,
50 x 12), against the restatements of tests/raster_ref.py and tests/raster_raw_ref.py, which take pairs already:

- c2s_cut_windows, c2s_cut_windows_raw (int16 and float32 sources, with and without the compaction and the NDVI) and
  c2s_window_frames: bit for bit / exactly equal, every flip, two calls split inside a window row, one window more
  allocated than cut, which must stay NaN;
- c2s_softmax_blend + c2s_blend_finish, hann and flat: |proba - ref64| <= raster_ref.bar(count), bit-identical across batch
  sizes, top-1 equal wherever the two best classes are further apart than the bar;
- predict_raster end to end with the tame U-TAE on a 40 x 75 raster, both patch orientations, against the model's own B = 1
  logits on windows cut with torch slicing and blended in float64, at the same bar;
- c2s_softmax_stitch and predict_tile with h1 != w1 against oracle.tail_oracle.softmax_stitch, at that test's 1e-6.

Observed on an MI355X: blend max |proba - ref64| 1.1e-7 ... 2.4e-7 against bars of 2.5e-6 (M = 8) and 3.9e-6 (M = 16);
predict_raster 2.8e-8 and 2.7e-8 against 2.5e-6.  Found by these tests: nothing to fix.

The tests can fail: with inference._check_patch_stride returning (pw, ph, sx, sy) (a local patch, not part of the project;
a consistent swap, so every launch stays inside its tensors), both predict_raster cases and ten window_frames cases fail
here while test_raster_gpu.py and test_raster_raw_gpu.py pass unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

import raster_raw_ref as RW
import raster_ref as RR

pytestmark = pytest.mark.gpu

WINDOWS = [((16, 32), (12, 24)), ((32, 16), (24, 12))]
RASTERS = [(40, 75), (75, 40), (12, 50), (50, 12)]        # the last two: smaller than the window on one axis only
GEOMETRIES = [(hw, p, s) for p, s in WINDOWS for hw in RASTERS]
IDS = [f"{hw[0]}x{hw[1]}-patch{p[0]}x{p[1]}" for hw, p, s in GEOMETRIES]
CS = 11
ORDER = [2, 1, 0, 4, 5, 6, 3, 7, 8, 10]
NDVI = (7, 2)
_rng = np.random.default_rng(11)
MEAN = _rng.uniform(500, 3000, 10).astype(np.float32)
STD = _rng.uniform(300, 2000, 10).astype(np.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _counts(hw, patch, stride):
    return len(RR.window_origins(hw[0], patch[0], stride[0])), len(RR.window_origins(hw[1], patch[1], stride[1]))


def _smaller(hw, patch):
    return hw[0] < patch[0] or hw[1] < patch[1]


def test_geometries_are_what_the_docstring_says():
    for hw, patch, stride in GEOMETRIES:
        assert patch[0] != patch[1] and stride[0] != stride[1]
        assert (hw[0] < patch[0]) + (hw[1] < patch[1]) == (1 if hw in RASTERS[2:] else 0)
        ny, nx = _counts(hw, patch, stride)
        assert ny * nx > 1
    assert {_counts(hw, p, s) for hw, p, s in GEOMETRIES if hw == (40, 75)} == {(3, 3), (2, 6)}


# ---------------------------------------------------------------------------------------------------------------------
# the cuts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,patch,stride", GEOMETRIES, ids=IDS)
def test_cut_windows_bit_exact_rect(hw, patch, stride):
    from crop2seg_amd._lib import check, lib
    (H, W), (ph, pw), (sy, sx) = hw, patch, stride
    T, C = 2, 10
    rng = np.random.default_rng(H * 100 + W)
    series = rng.normal(0, 1, (T, C, H, W)).astype(np.float32)
    fill = (np.arange(C, dtype=np.float32) - 3.5) if _smaller(hw, patch) else None
    fill_a = None if fill is None else (ctypes.c_float * C)(*[float(v) for v in fill])
    ny, nx = _counts(hw, patch, stride)
    n = ny * nx
    split = nx // 2 + 1
    sd = torch.from_numpy(series).cuda()
    for flip in range(4):
        ref = RR.cut_windows(series, patch, stride, flip, fill)
        assert ref.shape == (n, T, C, ph, pw)
        x = torch.full((n + 1, T, C, ph, pw), float("nan"), device="cuda")       # one window more: must stay untouched
        for first, cnt in ((0, split), (split, n - split)):
            if cnt:
                check(lib().c2s_cut_windows(sd.data_ptr(), x[first:].data_ptr(), T, C, H, W, ph, pw, sy, sx, first, cnt, flip,
                                            fill_a, _stream()), "cut_windows")
        got = x.cpu().numpy()
        assert np.array_equal(got[:n].view(np.uint32), ref.view(np.uint32)), (hw, patch, stride, flip)
        assert bool(np.isnan(got[n]).all()), "the cut wrote past its windows"


def _code(a):
    from crop2seg_amd import _lib
    return {np.dtype(np.float32): _lib.SRC_F32, np.dtype(np.int16): _lib.SRC_I16}[a.dtype]


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("hw,patch,stride", GEOMETRIES, ids=IDS)
def test_window_frames_exact_rect(hw, patch, stride, dtype):
    from crop2seg_amd._lib import check, lib
    from crop2seg_amd.inference import window_frames
    (H, W), (ph, pw), (sy, sx) = hw, patch, stride
    T = 5
    a = RW.scene(dtype, T, CS, H, W, seed=H + T)
    dates = 3 + 5 * np.arange(T, dtype=np.int64)
    src, dd = torch.from_numpy(a).cuda(), torch.from_numpy(dates).cuda()
    ny, nx = _counts(hw, patch, stride)
    nw = ny * nx
    split = nx // 2 + 1
    for permille in (0, 250, 1000):
        ref = RW.window_frames(a, dates, patch, stride, 0, permille)
        slots = torch.full((nw, T), -9, dtype=torch.int32, device="cuda")
        counts = torch.full((nw,), -9, dtype=torch.int32, device="cuda")
        wd = torch.full((nw, T), -9, dtype=torch.int64, device="cuda")
        px = torch.full((nw, T), -9, dtype=torch.int32, device="cuda")
        for first, n in ((0, split), (split, nw - split)):
            if n:
                check(lib().c2s_window_frames(src.data_ptr(), _code(a), dd.data_ptr(), px[first:].data_ptr(),
                                              slots[first:].data_ptr(), counts[first:].data_ptr(), wd[first:].data_ptr(), T, CS, H, W,
                                              ph, pw, sy, sx, first, n, 0.0, permille, _stream()), "window_frames")
        for g, r, name in zip((slots, counts, wd, px), ref, ("slots", "counts", "win_dates", "nodata_px")):
            assert np.array_equal(g.cpu().numpy(), r), (name, hw, patch, permille)
    ref = RW.window_frames(a, dates, patch, stride, 0, 250)
    assert ref[1].min() < T, "some window drops a frame"
    for g, r in zip(window_frames(src, torch.from_numpy(dates), patch, stride, 0, 250), ref):       # the public function
        assert np.array_equal(g.cpu().numpy(), r)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("hw,patch,stride", GEOMETRIES, ids=IDS)
def test_cut_windows_raw_bit_exact_rect(hw, patch, stride, dtype):
    from crop2seg_amd._lib import check, lib
    (H, W), (ph, pw), (sy, sx) = hw, patch, stride
    T = 3
    a = RW.scene(dtype, T, CS, H, W, seed=T + W)
    ny, nx = _counts(hw, patch, stride)
    n = ny * nx
    split = nx // 2 + 1
    slots = RW.window_frames(a, np.arange(T), patch, stride, 0, 250)[0]
    small = _smaller(hw, patch)
    f10 = [0.5 * c - 2.0 for c in range(10)] if small else None
    f11 = [0.25 * c + 1.0 for c in range(11)] if small else None
    cases = [(dict(order=ORDER, mean=MEAN, std=STD, fill=f10, pad_value=-3.5, ndvi=None), slots),
             (dict(order=ORDER, mean=None, std=None, fill=f11, pad_value=0.0, ndvi=NDVI), None)]
    fa = lambda v: None if v is None else (ctypes.c_float * len(v))(*[float(f) for f in v])
    src = torch.from_numpy(a).cuda()
    for kw, sl in cases:
        C = len(kw["order"]) + (1 if kw["ndvi"] else 0)
        sd = None if sl is None else torch.from_numpy(sl).cuda()
        na, nb = kw["ndvi"] if kw["ndvi"] else (-1, -1)
        for flip in range(4):
            ref = RW.cut_windows_raw(a, patch, stride, flip, slots=sl, **kw)
            x = torch.full((n + 1, T, C, ph, pw), float("nan"), device="cuda")
            for first, cnt in ((0, split), (split, n - split)):
                if cnt:
                    check(lib().c2s_cut_windows_raw(src.data_ptr(), _code(a), x[first:].data_ptr(),
                                                    None if sd is None else sd[first:].data_ptr(), T, C, CS, H, W, ph, pw, sy, sx,
                                                    first, cnt, flip, (ctypes.c_int * len(ORDER))(*ORDER), fa(kw["mean"]),
                                                    fa(kw["std"]), fa(kw["fill"]), kw["pad_value"], na, nb, _stream()),
                          "cut_windows_raw")
            got = x.cpu().numpy()
            assert np.array_equal(got[:n].view(np.uint32), ref.view(np.uint32)), (a.dtype, hw, patch, flip, C, sl is not None)
            assert bool(np.isnan(got[n]).all()), "the cut wrote past its windows"


# ---------------------------------------------------------------------------------------------------------------------
# the blend
# ---------------------------------------------------------------------------------------------------------------------
def _feed(ld, acc, wsum, ty, tx, first, cnt, K, hw, patch, stride, flip):
    from crop2seg_amd._lib import check, lib
    check(lib().c2s_softmax_blend(ld[first:first + cnt].contiguous().data_ptr(), acc.data_ptr(), wsum.data_ptr(),
                                  None if ty is None else ty.data_ptr(), None if tx is None else tx.data_ptr(), first, cnt, K,
                                  patch[0], patch[1], hw[0], hw[1], stride[0], stride[1], flip, _stream()), "softmax_blend")


@pytest.mark.parametrize("window", ["hann", "flat"])
@pytest.mark.parametrize("hw,patch,stride", GEOMETRIES, ids=IDS)
def test_blend_matches_fp64_and_is_batch_invariant_rect(hw, patch, stride, window):
    from crop2seg_amd._lib import check, lib
    (H, W), (ph, pw) = hw, patch
    K = 15
    ny, nx = _counts(hw, patch, stride)
    n = ny * nx
    g = torch.Generator().manual_seed(13 + H)
    passes = [(RR.FLIPS[f], RR.random_logits(g, (n, K, ph, pw))) for f in ("", "h", "v", "hv")]
    wy, wx = (RR.hann(ph), RR.hann(pw)) if window == "hann" else (None, None)
    ty = None if wy is None else torch.from_numpy(wy).cuda()
    tx = None if wx is None else torch.from_numpy(wx).cuda()
    rp, rt, count = RR.blend([(f, l.numpy()) for f, l in passes], H, W, patch, stride, wy, wx)
    bound = RR.bar(count)
    dev = [(f, l.cuda()) for f, l in passes]
    results = []
    for bs in (1, 4, n):
        acc = torch.full((K, H, W), float("nan"), device="cuda")
        wsum = torch.full((H, W), float("nan"), device="cuda")
        check(lib().c2s_fill(acc.data_ptr(), acc.numel(), 0.0, _stream()), "fill")
        check(lib().c2s_fill(wsum.data_ptr(), wsum.numel(), 0.0, _stream()), "fill")
        for f, ld in dev:                                                    # flips outer, window batches inner
            for first in range(0, n, bs):
                _feed(ld, acc, wsum, ty, tx, first, min(bs, n - first), K, hw, patch, stride, f)
        top1 = torch.full((H, W), -1, device="cuda", dtype=torch.int64)
        check(lib().c2s_blend_finish(acc.data_ptr(), wsum.data_ptr(), top1.data_ptr(), K, H, W, _stream()), "blend_finish")
        results.append((acc.cpu(), top1.cpu()))
    for p, t in results[1:]:
        assert torch.equal(p, results[0][0]) and torch.equal(t, results[0][1]), "the blend must not depend on the batch size"
    proba, top1 = results[0]
    err = float(np.abs(proba.numpy().astype(np.float64) - rp).max())
    print(f"blend {hw} patch {patch} stride {stride} {window}: M = {int(count.max())}, max |proba - ref64| = {err:.3e}, "
          f"bar {bound:.3e}")
    assert err <= bound
    agree = top1.numpy() == rt
    top2 = np.sort(rp, axis=0)[-2:]
    assert bool(agree[(top2[1] - top2[0]) > bound].all()) and float(agree.mean()) > 0.99


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tame_utae():
    import crop2seg_amd as C2S
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=[32, 15])
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    return net.cuda().eval()


def _model_reference(net, series, dates, patch, stride, flips, fill):
    """test_raster_gpu._model_reference for pairs: the model's own B = 1 logits on windows cut with torch slicing /
    torch.flip, blended by the float64 restatement under hann(ph) x hann(pw)."""
    T, C, H, W = series.shape
    (ph, pw), (sy, sx) = patch, stride
    passes = []
    with torch.no_grad():
        for f in flips:
            out = []
            for oy in RR.window_origins(H, ph, sy):
                for ox in RR.window_origins(W, pw, sx):
                    win = torch.full((T, C, ph, pw), float(fill))
                    src = series[:, :, oy:oy + ph, ox:ox + pw]
                    win[:, :, :src.shape[2], :src.shape[3]] = src
                    dims = [d for d, ch in ((2, "v"), (3, "h")) if ch in f]
                    if dims:
                        win = torch.flip(win, dims)
                    logits = net(win[None].contiguous().cuda(), batch_positions=dates[None].cuda())[0]
                    assert logits.shape == (15, ph, pw)
                    out.append(logits.cpu().numpy())
            passes.append((RR.FLIPS[f], np.stack(out)))
    return RR.blend(passes, H, W, patch, stride, RR.hann(ph), RR.hann(pw))


@pytest.mark.parametrize("patch,stride", WINDOWS, ids=["patch16x32", "patch32x16"])
def test_predict_raster_end_to_end_rect(tame_utae, patch, stride):
    from crop2seg_amd.inference import predict_raster
    H, W, T = 40, 75, 4
    g = torch.Generator().manual_seed(29 + H)
    series = torch.randn(T, 10, H, W, generator=g)
    dates = 5 * torch.arange(T)
    flips = ("h", "v")
    rp, rt, count = _model_reference(tame_utae, series, dates, patch, stride, flips, 0.0)
    bound = RR.bar(count)
    sd, dd = series.cuda(), dates.cuda()
    proba, top1 = predict_raster(tame_utae, sd, dd, patch=patch, stride=stride, window="hann", batch_size=5, flips=flips)
    assert proba.shape == (15, H, W) and top1.shape == (H, W)
    err = float(np.abs(proba.cpu().numpy().astype(np.float64) - rp).max())
    print(f"predict_raster patch {patch} stride {stride}: M = {int(count.max())}, max |proba - ref64| = {err:.3e}, bar {bound:.3e}")
    assert err <= bound
    top2 = np.sort(rp, axis=0)[-2:]
    assert bool((top1.cpu().numpy() == rt)[(top2[1] - top2[0]) > bound].all())
    p, t = predict_raster(tame_utae, sd, dd, patch=patch, stride=stride, window="hann", batch_size=1, flips=flips)
    assert torch.equal(p, proba) and torch.equal(t, top1), "predict_raster must not depend on batch_size"


# ---------------------------------------------------------------------------------------------------------------------
# the stitch of predict_tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h1,w1", [(16, 32), (32, 16)])
def test_softmax_stitch_rect(h1, w1):
    from oracle import tail_oracle as TO
    from crop2seg_amd._lib import check, lib
    g = torch.Generator().manual_seed(13)
    grid, K = 3, 15
    out_h, out_w = grid * h1 - 7, grid * w1 - 13                    # a crop inside the last row / column of patches
    logits = RR.random_logits(g, (grid * grid, K, h1, w1))
    rp, rt = TO.softmax_stitch([l[None] for l in logits], grid=grid, crop=grid * max(h1, w1))
    assert rp.shape == (K, grid * h1, grid * w1)
    rp, rt = rp[:, :out_h, :out_w], rt[:out_h, :out_w]
    proba = torch.full((K, out_h, out_w), -1.0, device="cuda")
    top1 = torch.full((out_h, out_w), -1, device="cuda", dtype=torch.int64)
    ld = logits.cuda()
    for first, n in ((0, 4), (4, 5)):                             # two batches of patches
        check(lib().c2s_softmax_stitch(ld[first:first + n].contiguous().data_ptr(), proba.data_ptr(), top1.data_ptr(), first, n, K,
                                       h1, w1, grid, out_h, out_w, _stream()), "softmax_stitch")
    assert float((proba.cpu() - rp).abs().max()) <= 1e-6
    agree = (top1.cpu() == rt)
    top2 = rp.topk(2, dim=0).values
    assert bool(agree[(top2[0] - top2[1]) > 1e-6].all()) and float(agree.float().mean()) > 0.99


def test_predict_tile_rect(tame_utae):
    from oracle import tail_oracle as TO
    from crop2seg_amd.inference import predict_tile
    grid, h1, w1, T, crop = 3, 32, 16, 4, 90
    g = torch.Generator().manual_seed(17)
    x = torch.randn(grid * grid, T, 10, h1, w1, generator=g).cuda()
    dates = (5 * torch.arange(T))[None].repeat(grid * grid, 1).cuda()
    proba, top1 = predict_tile(tame_utae, x, dates, grid=grid, crop=crop, batch_size=4)
    with torch.no_grad():
        singles = [tame_utae(x[i:i + 1].contiguous(), batch_positions=dates[i:i + 1].contiguous()).cpu() for i in range(grid * grid)]
    rp, rt = TO.softmax_stitch(singles, grid=grid, crop=crop)
    assert proba.shape == rp.shape == (15, 90, 48)
    assert float((proba.cpu() - rp).abs().max()) <= 1e-6
    top2 = rp.topk(2, dim=0).values
    assert bool((top1.cpu() == rt)[(top2[0] - top2[1]) > 1e-6].all())
