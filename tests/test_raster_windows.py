"""CPU checks of overlapped sliding-window inference: the library's window placement against tests/raster_ref.py, the
argument checks of the three entry points before any launch, the reference's own check (scatter == per-pixel loop, two
planted faults detected), and predict_raster's argument handling."""
import numpy as np
import pytest
import torch

import raster_ref as RR


@pytest.mark.parametrize("patch", [16, 32])
def test_window_placement_matches_reference(patch):
    from crop2seg_amd import _lib
    L = _lib.lib()
    for stride in range(1, patch + 1):
        most = -(-patch // stride) + 1
        for size in range(1, 3 * patch + 1):
            ref = RR.window_origins(size, patch, stride)
            n = L.c2s_window_count(size, patch, stride)
            assert n == len(ref), (size, patch, stride)
            got = [L.c2s_window_origin(i, size, patch, stride) for i in range(n)]
            assert got == ref, (size, patch, stride)
            assert all(b >= a for a, b in zip(got, got[1:])), "origins must not decrease"
            assert got[0] == 0 and got[-1] == max(size - patch, 0)
            cover = np.zeros(size, np.int64)
            for o in got:
                cover[o:o + patch] += 1
            assert cover.min() >= 1, "every pixel is covered"
            assert cover.max() <= most, (size, patch, stride, int(cover.max()))


def test_argument_validation_without_gpu():
    """Bad arguments return a negative value / C2S_EINVAL (-1) with a message naming the entry point, before any launch."""
    from crop2seg_amd import _lib
    L = _lib.lib()
    p = 4096                                                   # a non-NULL, 16-byte aligned stand-in: never dereferenced

    def refused(rc, word):
        return rc == -1 and word in L.c2s_last_error()

    assert refused(L.c2s_window_count(40, 16, 0), b"window_count") and refused(L.c2s_window_count(40, 16, 17), b"window_count")
    assert refused(L.c2s_window_count(0, 16, 8), b"window_count") and refused(L.c2s_window_count(40, 0, 1), b"window_count")
    assert refused(L.c2s_window_origin(0, 40, 16, 0), b"window_origin") and refused(L.c2s_window_origin(0, 40, 16, 17), b"window_origin")
    assert refused(L.c2s_window_origin(-1, 40, 16, 8), b"window_origin") and refused(L.c2s_window_origin(4, 40, 16, 8), b"window_origin")
    assert L.c2s_window_origin(3, 40, 16, 8) == 24

    ok = dict(T=2, C=10, H=37, W=45, ph=16, pw=16, sy=12, sx=12, first=0, n=3, flip=0)

    def cut(series=p, x=p, **kw):
        a = dict(ok, **kw)
        return L.c2s_cut_windows(series, x, a["T"], a["C"], a["H"], a["W"], a["ph"], a["pw"], a["sy"], a["sx"], a["first"], a["n"],
                                 a["flip"], None, None)

    assert refused(cut(series=None), b"cut_windows: null") and refused(cut(x=None), b"cut_windows: null")
    assert refused(cut(sy=0), b"cut_windows") and refused(cut(sx=17), b"cut_windows") and b"stride" in L.c2s_last_error()
    assert refused(cut(ph=20), b"cut_windows") and refused(cut(pw=12), b"cut_windows") and refused(cut(ph=8, sy=8), b"cut_windows")
    assert refused(cut(C=17), b"cut_windows") and b"C <= 16" in L.c2s_last_error()
    assert refused(cut(H=0), b"cut_windows") and refused(cut(T=0), b"cut_windows")
    assert refused(cut(flip=4), b"cut_windows") and refused(cut(flip=-1), b"cut_windows")
    assert refused(cut(first=-1), b"cut_windows") and refused(cut(n=0), b"cut_windows")
    assert refused(cut(first=10, n=3), b"cut_windows")          # 3 x 4 = 12 windows: 10 + 3 runs past the last

    okb = dict(first=0, n=3, K=15, ph=16, pw=16, H=37, W=45, sy=12, sx=12, flip=0)

    def blend(logits=p, acc=p, wsum=p, **kw):
        a = dict(okb, **kw)
        return L.c2s_softmax_blend(logits, acc, wsum, None, None, a["first"], a["n"], a["K"], a["ph"], a["pw"], a["H"], a["W"],
                                   a["sy"], a["sx"], a["flip"], None)

    assert refused(blend(logits=None), b"softmax_blend: null") and refused(blend(acc=None), b"softmax_blend: null")
    assert refused(blend(wsum=None), b"softmax_blend: null")
    assert refused(blend(sy=0), b"softmax_blend") and refused(blend(sx=17), b"softmax_blend") and b"stride" in L.c2s_last_error()
    assert refused(blend(K=0), b"softmax_blend") and refused(blend(K=33), b"softmax_blend") and b"K <= 32" in L.c2s_last_error()
    assert refused(blend(flip=4), b"softmax_blend") and refused(blend(H=0), b"softmax_blend")
    assert refused(blend(first=12, n=1), b"softmax_blend") and refused(blend(n=0), b"softmax_blend")

    assert refused(L.c2s_blend_finish(None, p, p, 15, 37, 45, None), b"blend_finish: null")
    assert refused(L.c2s_blend_finish(p, None, None, 15, 37, 45, None), b"blend_finish: null")
    assert refused(L.c2s_blend_finish(p, p, None, 0, 37, 45, None), b"blend_finish") and refused(L.c2s_blend_finish(p, p, None, 15, 0, 45, None), b"blend_finish")


def _small_case():
    """3 x 2 windows of 8 x 8 on an 18 x 13 raster, stride (6, 6): both axes end in a clamped window; K = 3, two passes."""
    H, W, patch, stride = 18, 13, (8, 8), (6, 6)
    assert (len(RR.window_origins(H, 8, 6)), len(RR.window_origins(W, 8, 6))) == (3, 2)
    g = torch.Generator().manual_seed(7)
    passes = [(f, RR.random_logits(g, (6, 3, 8, 8)).numpy()) for f in (0, 3)]
    return passes, H, W, patch, stride


def test_reference_blend_equals_per_pixel_loop():
    passes, H, W, patch, stride = _small_case()
    wy, wx = RR.hann(8), RR.hann(8)
    for ty, tx in ((None, None), (wy, wx)):
        p, t, c = RR.blend(passes, H, W, patch, stride, ty, tx)
        bp, bt, bc = RR.blend_per_pixel(passes, H, W, patch, stride, ty, tx)
        assert np.array_equal(c, bc) and c.min() >= 2 and c.max() == 8          # 2 passes x up to 2 x 2 windows
        assert float(np.abs(p - bp).max()) <= 1e-14 and np.array_equal(t, bt)
        assert float(np.abs(p.sum(0) - 1).max()) <= 1e-14


@pytest.mark.parametrize("fault", ["no_clamp", "no_unmirror"])
def test_reference_comparison_detects_planted_faults(fault):
    passes, H, W, patch, stride = _small_case()
    wy, wx = RR.hann(8), RR.hann(8)
    bp, _, bc = RR.blend_per_pixel(passes, H, W, patch, stride, wy, wx)
    p, _, c = RR.blend(passes, H, W, patch, stride, wy, wx, fault=fault)
    assert float(np.abs(p - bp).max()) > 1e-3, f"the comparison must see the planted fault {fault}"
    if fault == "no_clamp":
        assert not np.array_equal(c, bc)


def test_cut_reference_on_a_known_case():
    s = np.arange(2 * 1 * 5 * 7, dtype=np.float32).reshape(2, 1, 5, 7)
    w = RR.cut_windows(s, (4, 4), (3, 3), flip=0)
    assert w.shape == (4, 2, 1, 4, 4)                                       # origins (0, 1) x (0, 3)
    assert np.array_equal(w[3], s[:, :, 1:5, 3:7])
    assert np.array_equal(RR.cut_windows(s, (4, 4), (3, 3), flip=3)[1], s[:, :, 0:4, 3:7][:, :, ::-1, ::-1])
    small = RR.cut_windows(s, (8, 8), (8, 8), flip=1, fill=[-2.0])          # raster smaller than the window
    assert small.shape == (1, 2, 1, 8, 8) and np.array_equal(small[0, :, :, :5, 1:], s[:, :, :, ::-1])
    assert float(small[0, :, :, 5:].max()) == -2.0 and float(small[0, :, :, :, 0].max()) == -2.0


class _Never(torch.nn.Module):
    def forward(self, *a, **k):
        raise AssertionError("the model must not run")

    def check_health(self):
        raise AssertionError("no launch, no health check")


def test_predict_raster_refuses_cpu_tensors():
    from crop2seg_amd.inference import predict_raster
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_raster(_Never(), torch.zeros(4, 10, 40, 40), torch.arange(4), patch=32, stride=24)


@pytest.mark.parametrize("kw", [dict(flips=("", "x")), dict(flips=()), dict(flips="hv"), dict(window="hamming"), dict(stride=0),
                                dict(stride=33), dict(stride=(24, 40)), dict(stride=(8, 8, 8)), dict(stride=1.5),
                                dict(patch=20), dict(patch=8, stride=8), dict(fill=[0.0, 1.0])])
def test_predict_raster_bad_arguments_raise_value_error(kw):
    from crop2seg_amd.inference import predict_raster
    args = dict(patch=32, stride=24)
    args.update(kw)
    model = _Never().train()
    with pytest.raises(ValueError, match="predict_raster"):
        predict_raster(model, torch.zeros(4, 10, 40, 40), torch.arange(4), **args)
    assert model.training


def test_taper_is_positive_and_symmetric():
    from crop2seg_amd.inference import taper
    for n in (16, 32, 128):
        w = taper("hann", n)
        assert w.dtype == torch.float32 and np.array_equal(w.numpy(), RR.hann(n))
        assert float(w.min()) > 0 and float(w.max()) <= 1 and float((w - w.flip(0)).abs().max()) <= 2.0 ** -24
    assert taper("flat", 16) is None
