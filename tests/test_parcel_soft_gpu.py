"""GPU checks of the soft parcel vote (csrc/parcels.hip `c2s_parcel_soft_vote`, postprocess.parcel_soft_vote) against
tests/parcel_soft_ref.py.  The kernel sums 2^-32 fixed-point probabilities in 64-bit integers, so with probabilities as
input every comparison is exact equality, means included (as bit patterns); under from_logits the float64 restatement is
the yardstick and only the means carry a tolerance (derived at the test)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parcel_ref as PR  # noqa: E402
import parcel_soft_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                      # guard bytes either side of a buffer (keeps the 16-byte alignment of the interior)
UNWRITTEN = int(np.frombuffer(b"\xf9" * 8, dtype=np.int64)[0])


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A device buffer of `nbytes` (rounded up to 16) with a sentinel-filled guard before and behind it."""

    def __init__(self, nbytes, fill=0xA5):
        self.nbytes, self.fill = -(-nbytes // 16) * 16, fill
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def body(self, dtype, count):
        return self.raw[GUARD:GUARD + self.nbytes].view(dtype)[:count]

    def intact(self):
        return bool((self.raw[:GUARD] == self.fill).all()) and bool((self.raw[GUARD + self.nbytes:] == self.fill).all())


def run_abi(scores, labels, cap, from_logits=False, bg_mean=0.7, outside="zero"):
    """c2s_parcel_soft_vote through the C ABI with guarded outputs and workspace, `out` prefilled with 0xF9 bytes ->
    the restatement's dict, plus `sums` (read back from the workspace) and `err` (the four error words)."""
    from crop2seg_amd._lib import check, lib
    L = lib()
    nb, k, h, w = scores.shape
    sd = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    ld = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    need = L.c2s_parcel_soft_vote_workspace_bytes(nb, cap, k)
    assert need >= nb * cap * (8 * k + 4) and need % 16 == 0
    out, ws = Guarded(8 * nb * h * w, fill=0xF9), Guarded(need)
    lab, top2, pix, mean = Guarded(4 * nb * cap), Guarded(4 * nb * cap), Guarded(4 * nb * cap), Guarded(4 * nb * cap * k)
    err = torch.zeros(4, dtype=torch.int32, device="cuda")
    check(L.c2s_parcel_soft_vote(sd.data_ptr(), ld.data_ptr(), out.ptr(), lab.ptr(), top2.ptr(), mean.ptr(), pix.ptr(), nb, k, h,
                                 w, cap, 1 if from_logits else 0, bg_mean, 1 if outside == "keep" else 0, ws.ptr(), need,
                                 err.data_ptr() + 4, _stream()), "parcel_soft_vote")
    torch.cuda.synchronize()
    assert all(g.intact() for g in (out, ws, lab, top2, pix, mean)), "a guard around an output or the workspace was written"
    i32 = lambda g: g.body(torch.int32, nb * cap).view(nb, cap).cpu().numpy()      # noqa: E731
    return dict(out=out.body(torch.int64, nb * h * w).view(nb, h, w).cpu().numpy(), label=i32(lab), top2=i32(top2),
                pixels=i32(pix), mean=mean.body(torch.float32, nb * cap * k).view(nb, cap, k).cpu().numpy(),
                sums=ws.body(torch.int64, nb * cap * k).view(nb, cap, k).cpu().numpy().astype(np.uint64), err=err.tolist())


def run_python(scores, labels, cap, from_logits=False, bg_mean=0.7, outside="zero"):
    from crop2seg_amd import postprocess as PP
    res = PP.parcel_soft_vote(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), bg_mean, from_logits, outside, cap)
    assert [t.dtype for t in res] == [torch.int64, torch.int32, torch.int32, torch.float32, torch.int32]
    return dict(zip(("out", "label", "top2", "mean", "pixels"), (t.cpu().numpy() for t in res)))


def both_entries_equal(scores, labels, cap, want, **kw):
    """The C ABI and the Python entry against the integer restatement, every field exactly."""
    got = run_abi(scores, labels, cap, **kw)
    assert got["err"] == [0, want["skipped"], 0, want["nonfinite"]]
    assert np.array_equal(got["sums"], want["sums"])
    assert SR.same_table(got, want)
    py = run_python(scores, labels, cap, **kw)
    skipped = (np.asarray(labels) < 0) | (np.asarray(labels) > cap)         # the Python entry's `out` is not prefilled
    py["out"] = np.where(skipped, want["out"], py["out"])
    assert SR.same_table(py, want)
    return got


@pytest.fixture(scope="module")
def scene16():
    """B = 2, K = 16, 96 x 100 probabilities: 9600 pixels per image are no multiple of 256; ten workgroups."""
    return SR.make_soft_scene(2, 16, 96, 100, seed=61)


# ------------------------------------------------------------------------------------------------ 1, 2: bit for bit
@pytest.mark.parametrize("outside", ["zero", "keep"])
def test_probabilities_bit_for_bit(outside, scene16):
    from crop2seg_amd import postprocess as PP
    p, labels, cap = scene16
    want = SR.soft_vote(p, labels, cap, outside=outside)
    used = want["pixels"] > 0
    assert used.sum() > 100 and (want["label"][used] == 0).any()            # background-led parcels above bg_mean ...
    assert (want["label"] == want["top2"])[used].any()                      # ... and below it: the runner-up takes them
    both_entries_equal(p, labels, cap, want, outside=outside)
    assert PP.check_errors() == (0, 0) and PP.nonfinite_scores() == 0


@pytest.mark.parametrize("k", [2, 15, 32])
def test_class_counts_at_their_edges(k):
    p, labels, cap = SR.make_soft_scene(2, k, 40, 72, seed=50 + k)
    for outside in ("zero", "keep"):
        both_entries_equal(p, labels, cap, SR.soft_vote(p, labels, cap, outside=outside), outside=outside)


# ------------------------------------------------------------------------------------------------ 3: ids inside a wave
@pytest.mark.parametrize("pattern", ["cycle64", "alternate", "five"])
def test_ids_interleaved_inside_a_wave(pattern):
    """B = 1, K = 16, 24 x 128.  cycle64: ids 1..64 along each row, every lane of a wave another parcel; alternate: two ids
    in turn; five: a pattern of five ids whose period does not divide 64, so the groups of a wave change from wave to wave."""
    xs = np.arange(24 * 128).reshape(1, 24, 128)
    ids = {"cycle64": xs % 64 + 1, "alternate": np.where(xs % 2 == 0, 3, 7), "five": np.array([2, 9, 4, 9, 1])[xs % 5]}[pattern]
    p, labels, cap = SR.make_soft_scene(1, 16, 24, 128, seed=71, labels=ids.astype(np.int32), cap=int(ids.max()) + 1)
    want = SR.soft_vote(p, labels, cap)
    assert want["pixels"].sum() == 24 * 128
    both_entries_equal(p, labels, cap, want)


# ------------------------------------------------------------------------------------------------ 4: contention, 64 bits
def test_one_parcel_under_contention_sums_exactly():
    """One parcel of 264 x 265 = 69,960 pixels; class 3 is exactly 1.0 (q = 2^32: a 32-bit q or accumulator loses it, a
    float accumulator stops counting at 2^24 pixels' worth of bits), class 5 exactly 1.5 * 2^-32 (q rounds to even: 2)."""
    h, w = 264, 265
    p = np.zeros((1, 16, h, w), dtype=np.float32)
    p[0, 3], p[0, 5] = 1.0, 1.5 * 2.0 ** -32
    labels = np.ones((1, h, w), dtype=np.int32)
    want = SR.soft_vote(p, labels, 1)
    got = both_entries_equal(p, labels, 1, want)
    n = h * w
    assert n == 69960 and got["pixels"].tolist() == [[n]]
    assert int(got["sums"][0, 0, 3]) == n << 32 and int(got["sums"][0, 0, 5]) == 2 * n
    assert got["mean"][0, 0, 3] == np.float32(1.0) and got["mean"][0, 0, 5] == np.float32(2.0 ** -31)
    assert got["label"].tolist() == [[3]] and got["top2"].tolist() == [[5]] and (got["out"] == 3).all()


# ------------------------------------------------------------------------------------------------ 5: rule edges
def rule_scene(bg):
    """K = 4, rows of 64 pixels, a parcel per row, exactly representable probabilities around bg_mean = bg."""
    p = np.zeros((1, 4, 5, 64), dtype=np.float32)
    labels = np.repeat(np.arange(1, 6, dtype=np.int32)[None, :, None], 64, 2)
    rest = np.float32(1) - np.float32(bg)
    p[0, 2, 0], p[0, 3, 0] = 0.5, 0.5                      # 1: classes 2 and 3 have equal sums: 2 first
    p[0, 0, 1], p[0, 2, 1] = bg, rest                      # 2: every pixel's p_0 equal to bg_mean: not greater -> t2
    p[0, 0, 2], p[0, 2, 2] = bg, rest                      # 3: the same with one pixel raised -> 0
    p[0, 0, 2, 40], p[0, 2, 2, 40] = 0.875, 0.125
    p[0, 0, 3], p[0, 1, 3] = 0.5, 0.5                      # 4: 0 and 1 tie: t1 = 0, not above bg_mean -> 1; top2 = 1
    p[0, 1, 4], p[0, 0, 4] = 0.625, 0.375                  # 5: the background second
    return p, labels, 5


@pytest.mark.parametrize("bg", [0.75, 0.7])
def test_rule_edges(bg):
    """bg = 0.75 is exact in binary; bg = 0.7 is the default, the float 0.7f: p_0 = 0.7f gives S_0 = n * 0.7f * 2^32 exactly
    (0.7f * 2^32 is an integer), equal to the bound and so not above it."""
    p, labels, cap = rule_scene(bg)
    kw = {} if bg == 0.7 else dict(bg_mean=bg)
    want = SR.soft_vote(p, labels, cap, **kw)
    assert want["label"][0].tolist() == [2, 2, 0, 1, 1] and want["top2"][0].tolist() == [3, 2, 2, 1, 0]
    got = both_entries_equal(p, labels, cap, want, **kw)
    assert got["label"][0].tolist() == [2, 2, 0, 1, 1] and got["top2"][0].tolist() == [3, 2, 2, 1, 0]
    planted = SR.soft_vote(p, labels, cap, ge=True, **kw)                   # `>=` would have been rejected here
    assert planted["label"][0, 1] == 0 and not SR.same_table(got, planted)


# ------------------------------------------------------------------------------------------------ 6: empty and skipped
def test_empty_ids_and_skipped_pixels():
    from crop2seg_amd import postprocess as PP
    ids = np.zeros((1, 8, 64), dtype=np.int32)
    ids[0, :3, :40], ids[0, 3:6, 10:], ids[0, 6:, 20:50] = 1, 2, 4         # ids 3 and 5 are carried by no pixel
    p, labels, cap = SR.make_soft_scene(1, 4, 8, 64, seed=81, labels=ids, cap=5)
    labels = labels.copy()
    labels[0, 7, 0], labels[0, 7, 63] = -1, cap + 1                          # outside [0, cap]: counted, left unwritten
    p = p.copy()
    p[0, 2, 0, 5], p[0, 0, 4, 30] = np.nan, np.inf                           # in parcels 1 and 2: counted, add nothing
    p[0, 1, 0, 50] = np.nan                                                  # no parcel: not counted
    PP.check_errors(), PP.nonfinite_scores()                                 # whatever earlier calls left behind
    for outside in ("zero", "keep"):
        want = SR.soft_vote(p, labels, cap, outside=outside, fill=UNWRITTEN)
        assert (want["skipped"], want["nonfinite"]) == (2, 2)
        assert want["pixels"][0].tolist() == [3 * 40 - 1, 3 * 54 - 1, 0, 2 * 30, 0]
        got = both_entries_equal(p, labels, cap, want, outside=outside)
        assert got["out"][0, 7, 0] == UNWRITTEN and got["out"][0, 7, 63] == UNWRITTEN
        assert got["out"][0, 0, 5] == got["label"][0, 0] and got["out"][0, 4, 30] == got["label"][0, 1]     # still written
        for f in ("label", "top2", "pixels"):
            assert got[f][0, [2, 4]].tolist() == [0, 0]
        assert not got["mean"][0, [2, 4]].any() and np.isfinite(got["mean"]).all()
        # the Python readers: check_errors keeps its 2-tuple and its three words, the new count has its own reader
        res = PP.check_errors()
        assert isinstance(res, tuple) and res == (2, 0)
        assert PP.nonfinite_scores() == 2 and PP.nonfinite_scores() == 0 and PP.check_errors() == (0, 0)


# ------------------------------------------------------------------------------------------------ 7: logits
def test_logits_against_float64():
    """B = 2, K = 16, 96 x 100, no borderline parcel (margin 1e-4).  Labels, top-2 and out equal the float64 restatement.
    Means within 1e-5 absolute: the fp32 softmax of K = 16 classes is off by at most about (K + 4) * 2^-24 = 1.2e-6 relative
    (the subtraction, expf, K - 1 additions, the division), the fixed-point sum adds 2^-33; 1e-5 is that with a margin of
    eight and stays ten times under the decision margin."""
    scores, labels, cap = SR.make_soft_scene(2, 16, 96, 100, seed=91, logits=True)
    for outside in ("zero", "keep"):
        want = SR.soft_vote64(scores, labels, cap, outside=outside, from_logits=True)
        for got in (run_abi(scores, labels, cap, from_logits=True, outside=outside),
                    run_python(scores, labels, cap, from_logits=True, outside=outside)):
            assert SR.same_table(got, want, fields=("out", "label", "top2", "pixels"))
            err = float(np.abs(got["mean"].astype(np.float64) - want["mean"]).max())
            print(f"logits, outside={outside}: max |mean - float64 mean| = {err:.3e}")
            assert err <= 1e-5
    assert (want["label"][want["pixels"] > 0] == 0).any()


# ------------------------------------------------------------------------------------------------ 8: reproducibility
def test_runs_are_bit_identical_and_images_independent():
    p, labels, cap = SR.make_soft_scene(3, 16, 48, 100, seed=101)
    fields = ("out", "label", "top2", "pixels", "mean")
    first, again = run_abi(p, labels, cap), run_abi(p, labels, cap)
    assert SR.same_table(first, again) and np.array_equal(first["sums"], again["sums"])
    for b in range(3):
        one = run_abi(p[b:b + 1], labels[b:b + 1], cap)
        assert SR.same_table(one, {f: first[f][b:b + 1] for f in fields})
    lg, _, _ = SR.make_soft_scene(3, 16, 48, 100, seed=102, logits=True, labels=labels, cap=cap)
    a, b_ = run_abi(lg, labels, cap, from_logits=True), run_abi(lg, labels, cap, from_logits=True)
    assert SR.same_table(a, b_) and np.array_equal(a["sums"], b_["sums"])


# ------------------------------------------------------------------------------------------------ 9: plumbing
def test_homogenize_soft_is_the_soft_vote(scene16):
    from crop2seg_amd import postprocess as PP
    p, labels, cap = scene16
    pd, ld = torch.from_numpy(p).cuda(), torch.from_numpy(labels).cuda()
    PP.check_errors()                                                       # whatever earlier calls left behind
    for outside in ("zero", "keep"):
        hom = PP.homogenize(pd, ld, 16, type_="soft", from_logits=False, outside=outside, cap=cap)
        assert hom.dtype == torch.int64 and torch.equal(hom, PP.parcel_soft_vote(pd, ld, 0.7, False, outside, cap)[0])
        assert torch.equal(PP.homogenize(pd, ld, 16, type_="soft", from_logits=False, outside=outside), hom)    # default cap
    base = PP.homogenize(pd, ld, 16, type_="soft", from_logits=False)
    assert np.array_equal(base.cpu().numpy(), SR.soft_vote(p, labels, cap)["out"])
    low = PP.homogenize(pd, ld, 16, type_="soft", from_logits=False, bg_mean=0.45, cap=cap)
    assert np.array_equal(low.cpu().numpy(), SR.soft_vote(p, labels, cap, bg_mean=0.45)["out"]) and not torch.equal(low, base)
    one = PP.parcel_soft_vote(pd[1], ld[1], from_logits=False, cap=cap)                                       # [K,H,W] is B = 1
    assert [tuple(t.shape) for t in one] == [(96, 100), (cap,), (cap,), (cap, 16), (cap,)]
    assert SR.same_table(dict(zip(("out", "label", "top2", "mean", "pixels"), (t.cpu().numpy()[None] for t in one))),
                         SR.soft_vote(p[1:], labels[1:], cap))
    top1 = pd.argmax(1)                                                                                       # the hard path
    assert np.array_equal(PP.homogenize(top1, ld, 16).cpu().numpy(), PR.homogenize(top1.cpu().numpy(), labels, 16))
    assert PP.check_errors() == (0, 0)


def _tame(out_conv):
    import crop2seg_amd as C2S
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=out_conv)
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    return net.cuda().eval()


def _soft_of(proba, parcels, cap=None):
    from crop2seg_amd import postprocess as PP
    return PP.parcel_soft_vote(proba, parcels, from_logits=False, cap=cap)[0]


def test_predict_raster_soft_mode():
    """The tiny model and raster of tests/test_raster_gpu.py."""
    from crop2seg_amd.inference import predict_raster
    net = _tame([32, 16])
    g = torch.Generator().manual_seed(31)
    series = torch.randn(4, 10, 75, 90, generator=g).cuda()
    dates = (5 * torch.arange(4)).cuda()
    parcels = torch.zeros(75, 90, dtype=torch.int32)
    parcels[5:40, 8:50], parcels[45:70, 30:85] = 1, 2
    parcels = parcels.cuda()
    plain = predict_raster(net, series, dates, patch=32, stride=24)
    assert isinstance(plain, tuple) and len(plain) == 2
    proba, top1, hard = predict_raster(net, series, dates, patch=32, stride=24, parcels=parcels)
    p2, t2, soft = predict_raster(net, series, dates, patch=32, stride=24, parcels=parcels, parcel_mode="soft")
    assert torch.equal(p2, plain[0]) and torch.equal(t2, plain[1]) and torch.equal(proba, plain[0]) and torch.equal(top1, plain[1])
    assert soft.shape == (75, 90) and soft.dtype == torch.int64 and torch.equal(soft, _soft_of(proba, parcels))
    want = SR.soft_vote(proba.cpu().numpy()[None], parcels.cpu().numpy()[None], 2)
    assert np.array_equal(soft.cpu().numpy(), want["out"][0])
    for mode, full in (("soft", soft), ("hard", hard)):                     # parcel_cap: the same raster from a 2-row table
        assert torch.equal(predict_raster(net, series, dates, patch=32, stride=24, parcels=parcels, parcel_mode=mode,
                                          parcel_cap=2)[2], full)


def test_predict_tile_soft_mode():
    """The 2 x 2 tile of tests/test_parcel_gpu.py: 32 x 32 patches cropped to 60 x 60, K = 16."""
    from crop2seg_amd import postprocess as PP
    from crop2seg_amd.inference import predict_tile
    net = _tame([32, 16])
    grid, h1, T, crop = 2, 32, 4, 60
    g = torch.Generator().manual_seed(19)
    x = torch.randn(grid * grid, T, 10, h1, h1, generator=g).cuda()
    dates = (5 * torch.arange(T))[None].repeat(grid * grid, 1).cuda()
    parcels = torch.from_numpy(PR.label_components(PR.random_blobs(1, crop, crop, 47, cell=7), 1)[0][0]).cuda()
    plain = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4)
    assert isinstance(plain, tuple) and len(plain) == 2
    proba, top1, hard = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4, parcels=parcels)
    assert torch.equal(hard, PP.homogenize(top1, parcels, 16))              # the default is the hard vote, as it was
    p2, t2, soft = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4, parcels=parcels, parcel_mode="soft")
    assert torch.equal(p2, plain[0]) and torch.equal(t2, plain[1]) and torch.equal(proba, plain[0]) and torch.equal(top1, plain[1])
    assert torch.equal(soft, _soft_of(proba, parcels))
    cap = int(parcels.max())
    capped = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4, parcels=parcels, parcel_mode="soft", parcel_cap=cap)
    assert torch.equal(capped[2], soft)
    assert np.array_equal(soft.cpu().numpy(), SR.soft_vote(proba.cpu().numpy()[None], parcels.cpu().numpy()[None], cap)["out"][0])


def test_step_meters_soft_mode():
    """StepMeters.update(parcels=..., parcel_mode='soft'): the IoU meter sees the soft homogenisation of the logits; the
    top-2 and the loss meter are what they are without parcels."""
    from crop2seg_amd.learning.metrics import StepMeters
    from oracle import tail_oracle as TO
    K = 16
    logits, parcels, cap = SR.make_soft_scene(2, K, 64, 64, seed=111, logits=True)
    g = torch.Generator().manual_seed(41)
    y = torch.randint(0, K, (2, 64, 64), generator=g)
    want = SR.soft_vote64(logits, parcels, cap, from_logits=True)["out"]
    ld, pd = torch.from_numpy(logits).cuda(), torch.from_numpy(parcels).cuda()
    plain, hooked = StepMeters(K, ignore_index=-1), StepMeters(K, ignore_index=-1)
    loss = torch.tensor([0.5], device="cuda")
    plain.update(ld, y.cuda(), loss)
    pred, pred2 = hooked.update(ld, y.cuda(), loss, parcels=pd, parcel_mode="soft")
    assert np.array_equal(pred.cpu().numpy(), want) and not np.array_equal(want, logits.argmax(1))
    assert np.array_equal(hooked.iou.conf_metric.conf.cpu().numpy(), TO.confusion_matrix(want, y.numpy(), K))
    assert torch.equal(hooked.iou_top2.conf_metric.conf, plain.iou_top2.conf_metric.conf)
    assert hooked.loss_mean() == plain.loss_mean() == 0.5
    hard = StepMeters(K, ignore_index=-1)
    hard.update(ld, y.cuda(), loss, parcels=pd)                             # the default stays the hard vote
    assert np.array_equal(hard.iou.conf_metric.conf.cpu().numpy(),
                          TO.confusion_matrix(PR.homogenize(logits.argmax(1), parcels, K, 0.75, "zero"), y.numpy(), K))
