"""GPU checks of overlapped sliding-window inference: c2s_cut_windows bit for bit against tests/raster_ref.py,
c2s_softmax_blend + c2s_blend_finish against the float64 scatter restatement and bit-identical across batch sizes,
predict_raster == predict_tile on an exact-fit raster, predict_raster end to end against the model's own B = 1 logits, and
the boundary-head hook."""
import ctypes

import numpy as np
import pytest
import torch

import raster_ref as RR

pytestmark = pytest.mark.gpu

# (H, W), stride at patch 16: a clamped last window and W % 4 != 0; an exact fit; both axes smaller than the window
GEOMETRIES = [((37, 45), 12), ((32, 48), 16), ((10, 21), 12)]
PATCH = 16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nwin(H, W, patch, stride):
    return len(RR.window_origins(H, patch, stride)), len(RR.window_origins(W, patch, stride))


@pytest.mark.parametrize("hw,stride", GEOMETRIES)
def test_cut_windows_bit_exact(hw, stride):
    from crop2seg_amd._lib import check, lib
    H, W = hw
    T, C = 2, 10
    rng = np.random.default_rng(H * 100 + W)
    series = rng.normal(0, 1, (T, C, H, W)).astype(np.float32)
    fill = (np.arange(C, dtype=np.float32) - 3.5) if H < PATCH else None      # per-channel fill where the raster is smaller
    fill_a = None if fill is None else (ctypes.c_float * C)(*[float(v) for v in fill])
    ny, nx = _nwin(H, W, PATCH, stride)
    n = ny * nx
    split = nx // 2 + 1 if n > 1 else 1                                     # the first call ends inside a window row
    sd = torch.from_numpy(series).cuda()
    for flip in range(4):
        ref = RR.cut_windows(series, (PATCH, PATCH), (stride, stride), flip, fill)
        x = torch.full((n + 1, T, C, PATCH, PATCH), float("nan"), device="cuda")       # one window more: must stay untouched
        for first, cnt in ((0, split), (split, n - split)):
            if cnt:
                check(lib().c2s_cut_windows(sd.data_ptr(), x[first:].data_ptr(), T, C, H, W, PATCH, PATCH, stride, stride, first,
                                            cnt, flip, fill_a, _stream()), "cut_windows")
        got = x.cpu().numpy()
        assert np.array_equal(got[:n].view(np.uint32), ref.view(np.uint32)), (hw, stride, flip)
        assert bool(np.isnan(got[n]).all()), "the cut wrote past its windows"


def _feed(ld, acc, wsum, ty, tx, first, cnt, K, H, W, stride, flip):
    from crop2seg_amd._lib import check, lib
    check(lib().c2s_softmax_blend(ld[first:first + cnt].contiguous().data_ptr(), acc.data_ptr(), wsum.data_ptr(),
                                  None if ty is None else ty.data_ptr(), None if tx is None else tx.data_ptr(), first, cnt, K,
                                  PATCH, PATCH, H, W, stride, stride, flip, _stream()), "softmax_blend")


@pytest.mark.parametrize("window", ["hann", "flat"])
@pytest.mark.parametrize("hw,stride", GEOMETRIES)
def test_blend_matches_fp64_and_is_batch_invariant(hw, stride, window):
    from crop2seg_amd._lib import check, lib
    H, W = hw
    K = 15
    ny, nx = _nwin(H, W, PATCH, stride)
    n = ny * nx
    g = torch.Generator().manual_seed(13 + H)
    flips = ("", "h", "v", "hv")
    passes = [(RR.FLIPS[f], RR.random_logits(g, (n, K, PATCH, PATCH))) for f in flips]
    taper = RR.hann(PATCH) if window == "hann" else None
    ty = tx = None if taper is None else torch.from_numpy(taper).cuda()
    rp, rt, count = RR.blend([(f, l.numpy()) for f, l in passes], H, W, (PATCH, PATCH), (stride, stride), taper, taper)
    M = int(count.max())
    assert M == 4 * int(RR.blend([(0, passes[0][1].numpy())], H, W, (PATCH, PATCH), (stride, stride))[2].max())
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
                _feed(ld, acc, wsum, ty, tx, first, min(bs, n - first), K, H, W, stride, f)
        top1 = torch.full((H, W), -1, device="cuda", dtype=torch.int64)
        check(lib().c2s_blend_finish(acc.data_ptr(), wsum.data_ptr(), top1.data_ptr(), K, H, W, _stream()), "blend_finish")
        results.append((acc.cpu(), top1.cpu()))
    for p, t in results[1:]:
        assert torch.equal(p, results[0][0]) and torch.equal(t, results[0][1]), "the blend must not depend on the batch size"
    proba, top1 = results[0]
    err = float(np.abs(proba.numpy().astype(np.float64) - rp).max())
    print(f"blend {hw} stride {stride} {window}: M = {M}, max |proba - ref64| = {err:.3e}, bar {bound:.3e}")
    assert err <= bound
    agree = top1.numpy() == rt
    top2 = np.sort(rp, axis=0)[-2:]
    assert bool(agree[(top2[1] - top2[0]) > bound].all()) and float(agree.mean()) > 0.99
    # a NULL top1 leaves the probabilities the same
    acc2 = torch.zeros(K, H, W, device="cuda")
    ws2 = torch.zeros(H, W, device="cuda")
    for f, ld in dev:
        _feed(ld, acc2, ws2, ty, tx, 0, n, K, H, W, stride, f)
    check(lib().c2s_blend_finish(acc2.data_ptr(), ws2.data_ptr(), None, K, H, W, _stream()), "blend_finish")
    assert torch.equal(acc2.cpu(), proba)


@pytest.mark.parametrize("hw,stride", GEOMETRIES)
def test_blend_leaves_rows_outside_the_batch_untouched(hw, stride):
    """One batch of windows on accumulators full of a sentinel: rows outside [origin_y(first row), origin_y(last row) + patch)
    keep it bit for bit, for wsum and for every class of acc; inside, exactly the pixels under a window of the batch change."""
    H, W = hw
    K = 15
    ny, nx = _nwin(H, W, PATCH, stride)
    n = ny * nx
    g = torch.Generator().manual_seed(5)
    ld = RR.random_logits(g, (n, K, PATCH, PATCH)).cuda()
    oys, oxs = RR.window_origins(H, PATCH, stride), RR.window_origins(W, PATCH, stride)
    batches = [(0, 1), (n - 1, 1)] + ([(nx - 1, 3), (nx, nx)] if ny > 1 else [])
    for first, cnt in batches:
        acc = torch.full((K, H, W), 7.0, device="cuda")
        wsum = torch.full((H, W), 7.0, device="cuda")
        _feed(ld, acc, wsum, None, None, first, cnt, K, H, W, stride, 0)
        touched = np.zeros((H, W), bool)
        for w in range(first, first + cnt):
            oy, ox = oys[w // nx], oxs[w % nx]
            touched[oy:oy + PATCH, ox:ox + PATCH] = True
        ws, ac = wsum.cpu().numpy(), acc.cpu().numpy()
        assert np.array_equal(ws != 7.0, touched), (hw, first, cnt)
        assert bool((ac[:, ~touched] == 7.0).all()) and bool((ac[:, touched] > 7.0).all())
        y0, y1 = oys[first // nx], min(oys[(first + cnt - 1) // nx] + PATCH, H)
        assert not touched[:y0].any() and not touched[y1:].any()


@pytest.fixture(scope="module")
def tame_utae():
    import crop2seg_amd as C2S
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=[32, 15])
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    return net.cuda().eval()


def test_exact_fit_equals_predict_tile(tame_utae):
    """Stride = patch on a raster that the windows tile exactly, flat weights: the same patches through the same model, so
    predict_raster == predict_tile bit for bit."""
    from crop2seg_amd.inference import predict_raster, predict_tile
    grid, h1, T = 3, 32, 4
    g = torch.Generator().manual_seed(17)
    x = torch.randn(grid * grid, T, 10, h1, h1, generator=g)
    dates = 5 * torch.arange(T)
    series = x.view(grid, grid, T, 10, h1, h1).permute(2, 3, 0, 4, 1, 5).reshape(T, 10, grid * h1, grid * h1).contiguous()
    p0, t0 = predict_tile(tame_utae, x.cuda(), dates[None].repeat(grid * grid, 1).cuda(), grid=grid, crop=96, batch_size=4)
    p1, t1 = predict_raster(tame_utae, series.cuda(), dates.cuda(), patch=32, stride=32, window="flat", batch_size=4)
    assert p1.shape == (15, 96, 96) and t1.shape == (96, 96) and t1.dtype == torch.int64
    assert torch.equal(p1, p0) and torch.equal(t1, t0)


def _model_reference(net, series, dates, patch, stride, flips, window, fill):
    """The model's own B = 1 logits on windows cut with torch slicing / torch.flip, blended by the float64 restatement."""
    T, C, H, W = series.shape
    taper = RR.hann(patch) if window == "hann" else None
    fills = torch.as_tensor([fill] * C if isinstance(fill, float) else fill, dtype=torch.float32)
    passes = []
    with torch.no_grad():
        for f in flips:
            out = []
            for oy in RR.window_origins(H, patch, stride):
                for ox in RR.window_origins(W, patch, stride):
                    win = fills[None, :, None, None].repeat(T, 1, patch, patch)
                    src = series[:, :, oy:oy + patch, ox:ox + patch]
                    win[:, :, :src.shape[2], :src.shape[3]] = src
                    dims = [d for d, ch in ((2, "v"), (3, "h")) if ch in f]
                    if dims:
                        win = torch.flip(win, dims)
                    out.append(net(win[None].contiguous().cuda(), batch_positions=dates[None].cuda())[0].cpu().numpy())
            passes.append((RR.FLIPS[f], np.stack(out)))
    return RR.blend(passes, H, W, (patch, patch), (stride, stride), taper, taper)


@pytest.mark.parametrize("hw,fill", [((75, 90), 0.0), ((20, 40), [0.25 * c - 1.0 for c in range(10)])])
def test_predict_raster_end_to_end(tame_utae, hw, fill):
    from crop2seg_amd.inference import predict_raster
    H, W = hw
    T = 4
    g = torch.Generator().manual_seed(29 + H)
    series = torch.randn(T, 10, H, W, generator=g)
    dates = 5 * torch.arange(T)
    flips = ("", "h")
    rp, rt, count = _model_reference(tame_utae, series, dates, 32, 24, flips, "hann", fill)
    bound = RR.bar(count)
    sd, dd = series.cuda(), dates.cuda()
    tame_utae.train()                                                     # predict_raster restores the mode it found
    try:
        proba, top1 = predict_raster(tame_utae, sd, dd, patch=32, stride=24, window="hann", batch_size=5, flips=flips, fill=fill)
        assert tame_utae.training
    finally:
        tame_utae.eval()
    assert proba.shape == (15, H, W) and top1.shape == (H, W)
    err = float(np.abs(proba.cpu().numpy().astype(np.float64) - rp).max())
    print(f"predict_raster {hw}: M = {int(count.max())}, max |proba - ref64| = {err:.3e}, bar {bound:.3e}")
    assert err <= bound
    top2 = np.sort(rp, axis=0)[-2:]
    assert bool((top1.cpu().numpy() == rt)[(top2[1] - top2[0]) > bound].all())
    for bs in (1, 64):
        p, t = predict_raster(tame_utae, sd, dd, patch=32, stride=24, window="hann", batch_size=bs, flips=flips, fill=fill)
        assert torch.equal(p, proba) and torch.equal(t, top1), "predict_raster must not depend on batch_size"
        assert not tame_utae.training


def test_predict_raster_with_boundary_head():
    import crop2seg_amd as C2S
    from crop2seg_amd import postprocess
    from crop2seg_amd.inference import predict_raster
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=[32, 16], add_boundary_loss=True)
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(31)
    series = torch.randn(4, 10, 75, 90, generator=g).cuda()
    dates = (5 * torch.arange(4)).cuda()
    plain = predict_raster(net, series, dates, patch=32, stride=24)
    assert len(plain) == 2
    freq = np.bincount(plain[1].cpu().numpy().reshape(-1), minlength=16)
    code = int(np.argsort(-freq[1:], kind="stable")[1]) + 1              # a class the map holds, as test_predict_tile_with_parcels
    proba, top1, hom = predict_raster(net, series, dates, patch=32, stride=24, boundary_homogenize=True, boundary_code=code)
    assert torch.equal(proba, plain[0]) and torch.equal(top1, plain[1])
    want = postprocess.homogenize_boundaries(proba, boundary_code=code, from_logits=False)
    assert hom.shape == (75, 90) and hom.dtype == torch.int64 and torch.equal(hom, want)
    parcels = torch.zeros(75, 90, dtype=torch.int32)
    parcels[5:40, 8:50], parcels[45:70, 30:85] = 1, 2
    p4, t4, hom4 = predict_raster(net, series, dates, patch=32, stride=24, parcels=parcels.cuda())
    assert torch.equal(p4, proba) and torch.equal(hom4, postprocess.homogenize(top1, parcels.cuda(), 16))
    with pytest.raises(ValueError):
        predict_raster(net, series, dates, patch=32, stride=24, parcels=parcels.cuda(), boundary_homogenize=True)
