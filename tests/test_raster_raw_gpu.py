"""GPU checks of predict_raster on the stored series: c2s_window_frames exactly equal to tests/raster_raw_ref.py (all four
outputs), c2s_cut_windows_raw bit for bit (int16 / uint16 / float32, device and pinned sources, all flips, with and without
slots, inside the guard-band arena too), and predict_raster end to end: the raw path equal to the fp32 path on the
numpy-normalised series, unchanged by a nodata value that never occurs, and with planted empty frames against the model's
own B = 1 logits on the reference's compacted windows."""
import ctypes

import numpy as np
import pytest
import torch

import raster_raw_ref as RW
import raster_ref as RR
import redzone as RZ

pytestmark = pytest.mark.gpu

# (H, W), stride at patch 16: a clamped last window and odd W (rows start on odd 2-byte offsets); an exact fit; a raster
# smaller than the window
GEOMETRIES = [((37, 45), 12), ((32, 48), 16), ((10, 21), 12)]
PATCH = 16
CS = 11
ORDER = [2, 1, 0, 4, 5, 6, 3, 7, 8, 10]                                    # 11 source channels -> C = 10, not the identity
NDVI = (7, 2)                                                            # then C = 11
DTYPES = [np.int16, np.uint16, np.float32]
_rng = np.random.default_rng(11)
MEAN = _rng.uniform(500, 3000, 10).astype(np.float32)
STD = _rng.uniform(300, 2000, 10).astype(np.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(a):
    from crop2seg_amd import _lib
    return {np.dtype(np.float32): _lib.SRC_F32, np.dtype(np.int16): _lib.SRC_I16, np.dtype(np.uint16): _lib.SRC_U16}[a.dtype]


def _place(a, pinned=False):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory() if pinned else t.cuda()


def _nwin(H, W, stride):
    return len(RR.window_origins(H, PATCH, stride)) * len(RR.window_origins(W, PATCH, stride))


def _frames(src, a, dates_dev, stride, permille, first=0, n=None, out=None):
    """c2s_window_frames on windows [first, first + n) into (rows `first` .. of) the four outputs."""
    from crop2seg_amd._lib import check, lib
    T, Cs, H, W = a.shape
    nw = _nwin(H, W, stride)
    n = nw - first if n is None else n
    if out is None:
        out = (torch.full((nw, T), -9, dtype=torch.int32, device="cuda"), torch.full((nw,), -9, dtype=torch.int32, device="cuda"),
               torch.full((nw, T), -9, dtype=torch.int64, device="cuda"), torch.full((nw, T), -9, dtype=torch.int32, device="cuda"))
    slots, counts, wd, px = out
    check(lib().c2s_window_frames(src.data_ptr(), _code(a), dates_dev.data_ptr(), px[first:].data_ptr(), slots[first:].data_ptr(),
                                  counts[first:].data_ptr(), wd[first:].data_ptr(), T, Cs, H, W, PATCH, PATCH, stride, stride,
                                  first, n, 0.0, permille, _stream()), "window_frames")
    return out


@pytest.mark.parametrize("T", [3, 66])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,stride", GEOMETRIES)
def test_window_frames_exact(hw, stride, dtype, T):
    H, W = hw
    a = RW.scene(dtype, T, CS, H, W, seed=H + T)
    if dtype == np.int16:
        assert a.min() < 0
    if dtype == np.uint16:
        assert a.max() > 32767
    dates = 3 + 5 * np.arange(T, dtype=np.int64)
    src, dd = _place(a), torch.from_numpy(dates).cuda()
    nw = _nwin(H, W, stride)
    for permille in (0, 250, 1000):
        ref = RW.window_frames(a, dates, (PATCH, PATCH), (stride, stride), 0, permille)
        split = min(nw // 2 + 1, nw)                                            # two calls, split inside a window row
        out = _frames(src, a, dd, stride, permille, 0, split)
        if split < nw:
            out = _frames(src, a, dd, stride, permille, split, None, out)
        for g, r, name in zip(out, ref, ("slots", "counts", "win_dates", "nodata_px")):
            assert np.array_equal(g.cpu().numpy(), r), (name, hw, permille)
    last = RW.window_frames(a, dates, (PATCH, PATCH), (stride, stride), 0, 0)
    assert int(last[3][-1].min()) > 0 and last[1][-1] == 1, "the scene's last window has no complete frame: the fallback ran"
    if T > 5:
        assert int((last[3][-1] == last[3][-1].min()).sum()) > 1, "several frames tie for the fewest empty pixels"
        assert last[0][-1][0] == int(np.argmin(last[3][-1])), "the lowest t of the tie wins"


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_frames_exact_threshold_and_public_function(dtype):
    from crop2seg_amd.inference import window_frames
    a = RW.threshold_scene(dtype, T=3, Cs=CS)
    dates = np.array([4, 9, 30], np.int64)
    for permille, kept in ((250, [0, 2, -1]), (253, [0, 2, -1]), (254, [0, 1, 2]), (249, [2, -1, -1])):
        ref = RW.window_frames(a, dates, (PATCH, PATCH), (16, 16), 0, permille)
        assert ref[0][2].tolist() == kept and ref[3][2].tolist() == [64, 65, 0]
        got = window_frames(_place(a), torch.from_numpy(dates), PATCH, 16, 0, permille)
        for g, r in zip(got, ref):
            assert g.is_cuda and np.array_equal(g.cpu().numpy(), r) and g.cpu().numpy().dtype == r.dtype


def _cut(src, a, x, slots, first, n, stride, flip, order, mean, std, fill, pad_value, ndvi):
    from crop2seg_amd._lib import check, lib
    T, Cs, H, W = a.shape
    C = len(order) + (1 if ndvi else 0)
    fa = lambda v: None if v is None else (ctypes.c_float * len(v))(*[float(f) for f in v])
    na, nb = ndvi if ndvi else (-1, -1)
    check(lib().c2s_cut_windows_raw(src.data_ptr(), _code(a), x[first:].data_ptr(), None if slots is None else slots[first:].data_ptr(),
                                    T, C, Cs, H, W, PATCH, PATCH, stride, stride, first, n, flip, (ctypes.c_int * len(order))(*order),
                                    fa(mean), fa(std), fa(fill), pad_value, na, nb, _stream()), "cut_windows_raw")


def _cut_cases(a, stride):
    """(keyword arguments of the reference, slots or None): C = 10 normalised and C = 11 with NDVI, each with and without
    the compaction; a per-channel fill where the raster is smaller than the window."""
    T, Cs, H, W = a.shape
    slots = RW.window_frames(a, np.arange(T), (PATCH, PATCH), (stride, stride), 0, 250)[0]
    small = H < PATCH
    f10 = [0.5 * c - 2.0 for c in range(10)] if small else None
    f11 = [0.25 * c + 1.0 for c in range(11)] if small else None
    return [(dict(order=ORDER, mean=MEAN, std=STD, fill=f10, pad_value=0.0, ndvi=None), None),
            (dict(order=ORDER, mean=MEAN, std=STD, fill=f10, pad_value=-3.5, ndvi=None), slots),
            (dict(order=ORDER, mean=None, std=None, fill=f11, pad_value=0.0, ndvi=NDVI), None),
            (dict(order=ORDER, mean=MEAN, std=STD, fill=f11, pad_value=2.0, ndvi=NDVI), slots)]


def _run_cut_cases(a, stride, pinned=False, flips=range(4)):
    T, Cs, H, W = a.shape
    n = _nwin(H, W, stride)
    nx = len(RR.window_origins(W, PATCH, stride))
    split = nx // 2 + 1 if n > 1 else 1                                     # the first call ends inside a window row
    src = _place(a, pinned)
    for kw, slots in _cut_cases(a, stride):
        C = len(kw["order"]) + (1 if kw["ndvi"] else 0)
        sd = None if slots is None else torch.from_numpy(slots).cuda()
        for flip in flips:
            ref = RW.cut_windows_raw(a, (PATCH, PATCH), (stride, stride), flip, slots=slots, **kw)
            x = torch.full((n + 1, T, C, PATCH, PATCH), float("nan"), device="cuda")       # one window more: must stay untouched
            for first, cnt in ((0, split), (split, n - split)):
                if cnt:
                    _cut(src, a, x, sd, first, cnt, stride, flip, **kw)
            got = x.cpu().numpy()
            assert np.array_equal(got[:n].view(np.uint32), ref.view(np.uint32)), (a.dtype, (H, W), stride, flip, C, slots is not None)
            assert bool(np.isnan(got[n]).all()), "the cut wrote past its windows"


@pytest.mark.parametrize("T", [3, 66])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw,stride", GEOMETRIES)
def test_cut_windows_raw_bit_exact(hw, stride, dtype, T):
    _run_cut_cases(RW.scene(dtype, T, CS, *hw, seed=T + hw[1]), stride)


def test_pinned_source():
    """The source in pinned host memory: both entries read it in place."""
    (H, W), stride = GEOMETRIES[0]
    a = RW.scene(np.uint16, 3, CS, H, W, seed=2)
    _run_cut_cases(a, stride, pinned=True, flips=(0, 3))
    dates = np.array([1, 2, 3], np.int64)
    out = _frames(_place(a, pinned=True), a, torch.from_numpy(dates).cuda(), stride, 250)
    torch.cuda.synchronize()
    for g, r in zip(out, RW.window_frames(a, dates, (PATCH, PATCH), (stride, stride), 0, 250)):
        assert np.array_equal(g.cpu().numpy(), r)


@pytest.mark.parametrize("hw,stride", GEOMETRIES)
def test_both_entries_inside_the_guard_band_arena(hw, stride):
    from crop2seg_amd.inference import window_frames
    H, W = hw
    T = 66
    a = RW.scene(np.int16, T, CS, H, W, seed=9)
    dates = np.arange(T, dtype=np.int64)
    ref = RW.window_frames(a, dates, (PATCH, PATCH), (stride, stride), 0, 250)
    n = _nwin(H, W, stride)
    kw = dict(order=ORDER, mean=MEAN, std=STD, fill=None, pad_value=0.0, ndvi=NDVI)
    with RZ.arena("cuda", 64 * 1024 * 1024, copies=True) as arena:
        src = _place(a)
        got = window_frames(src, torch.from_numpy(dates), PATCH, stride, 0, 250)          # its four outputs are arena blocks
        assert all(arena.contains(g) for g in got)
        x = torch.empty(n, T, 11, PATCH, PATCH, device="cuda")
        assert arena.contains(x)
        for flip in (0, 3):
            _cut(src, a, x, got[0], 0, n, stride, flip, **kw)
            want = RW.cut_windows_raw(a, (PATCH, PATCH), (stride, stride), flip, slots=ref[0], **kw)
            assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert not bool(RZ.Arena.poisoned(x).any()), "every element of the windows is written"
        for g, r in zip(got, ref):
            assert np.array_equal(g.cpu().numpy(), r)
        arena.assert_intact()


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


E2E = dict(patch=32, stride=24, window="hann", flips=("", "h"))
E_MEAN = np.linspace(1800, 2600, 10).astype(np.float32)
E_STD = np.linspace(600, 1100, 10).astype(np.float32)


def _e2e_series(planted):
    """75 x 90, T = 4, 11 uint16 bands around 2200 +- 800 without a single 0; planted: frame 1 empty left of column 40, frame
    2 empty below row 60, and a 5 x 5 hole in frame 3."""
    rng = np.random.default_rng(41)
    a = np.clip(np.rint(rng.normal(2200, 800, (4, CS, 75, 90))), 1, 65535).astype(np.uint16)
    if planted:
        a[1, :, :, :40] = 0
        a[2, :, 60:, :] = 0
        a[3, :, 30:35, 50:55] = 0
    return a, torch.tensor([5, 30, 170, 300])


@pytest.fixture(scope="module")
def raw_result(tame_utae):
    """(a): the raw path on the uint16 series, batch size 5."""
    from crop2seg_amd.inference import predict_raster
    a, dates = _e2e_series(False)
    return predict_raster(tame_utae, _place(a), dates.cuda(), batch_size=5, channel_order=ORDER, mean=E_MEAN, std=E_STD, **E2E)


def test_raw_path_equals_fp32_path_on_the_normalised_series(tame_utae, raw_result):
    from crop2seg_amd.inference import predict_raster
    a, dates = _e2e_series(False)
    normalised = RW.convert(a, ORDER, E_MEAN, E_STD)
    p0, t0 = predict_raster(tame_utae, torch.from_numpy(normalised).cuda(), dates.cuda(), batch_size=5, **E2E)
    assert raw_result[0].shape == (15, 75, 90) and raw_result[1].dtype == torch.int64
    assert torch.equal(raw_result[0], p0) and torch.equal(raw_result[1], t0)
    src = _place(a)
    for bs in (1, 64):
        p, t = predict_raster(tame_utae, src, dates.cuda(), batch_size=bs, channel_order=ORDER, mean=E_MEAN, std=E_STD, **E2E)
        assert torch.equal(p, p0) and torch.equal(t, t0), "the raw path must not depend on batch_size"


def test_nodata_that_never_occurs_changes_nothing(tame_utae, raw_result):
    from crop2seg_amd.inference import predict_raster
    a, dates = _e2e_series(False)
    assert int((a == 0).sum()) == 0
    p, t = predict_raster(tame_utae, _place(a), dates.cuda(), batch_size=5, channel_order=ORDER, mean=E_MEAN, std=E_STD, nodata=0,
                          **E2E)
    assert torch.equal(p, raw_result[0]) and torch.equal(t, raw_result[1])


def test_planted_empty_frames_end_to_end(tame_utae):
    """The reference: the model's own B = 1 logits on the reference's windows (compacted frames, padded dates), blended by
    raster_ref.blend; |proba - ref| <= raster_ref.bar(count) on every pixel, top1 == first maximum of the returned proba on
    every pixel, bit-identical across batch sizes."""
    from crop2seg_amd.inference import predict_raster
    a, dates = _e2e_series(True)
    permille = 100
    st = (E2E["stride"],) * 2
    pt = (E2E["patch"],) * 2
    slots, counts, wd, _ = RW.window_frames(a, dates.numpy(), pt, st, 0, permille)
    assert counts.min() >= 1 and counts.min() < 4 and counts.max() == 4, "some windows lose frames, some keep all"
    passes = []
    with torch.no_grad():
        for f in E2E["flips"]:
            wins = RW.cut_windows_raw(a, pt, st, RR.FLIPS[f], ORDER, E_MEAN, E_STD, None, tame_utae.spec.pad_value, None, slots)
            out = [tame_utae(torch.from_numpy(wins[w:w + 1]).cuda(), batch_positions=torch.from_numpy(wd[w:w + 1]).cuda())[0]
                   .cpu().numpy() for w in range(wins.shape[0])]
            passes.append((RR.FLIPS[f], np.stack(out)))
    taper = RR.hann(E2E["patch"])
    rp, _, count = RR.blend(passes, 75, 90, pt, st, taper, taper)
    bound = RR.bar(count)
    src = _place(a)
    kw = dict(channel_order=ORDER, mean=E_MEAN, std=E_STD, nodata=0, max_nodata_permille=permille, **E2E)
    proba, top1 = predict_raster(tame_utae, src, dates.cuda(), batch_size=5, **kw)
    err = float(np.abs(proba.cpu().numpy().astype(np.float64) - rp).max())
    print(f"planted empty frames: kept {counts.tolist()}, M = {int(count.max())}, max |proba - ref64| = {err:.3e}, bar {bound:.3e}")
    assert err <= bound
    assert np.array_equal(top1.cpu().numpy(), proba.cpu().numpy().argmax(axis=0))
    for bs in (1, 64):
        p, t = predict_raster(tame_utae, src, dates.cuda(), batch_size=bs, **kw)
        assert torch.equal(p, proba) and torch.equal(t, top1), "predict_raster must not depend on batch_size"
    # dropping the frames matters: the same raster with every frame fed to every window gives another map
    p_all, _ = predict_raster(tame_utae, src, dates.cuda(), batch_size=5, channel_order=ORDER, mean=E_MEAN, std=E_STD, **E2E)
    assert not torch.equal(p_all, proba)
