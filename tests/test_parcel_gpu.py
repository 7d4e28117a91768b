"""GPU checks of the parcel homogenisation (csrc/parcels.hip, crop2seg_amd/postprocess.py) against tests/parcel_ref.py.
Everything after the seeds rule is integer work and the seeds inputs carry no borderline pixel, so every comparison is
exact equality; no tolerance appears."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parcel_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = PR.label_cases()
GUARD = 256                      # guard bytes either side of a buffer (keeps the 16-byte alignment of the interior)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """A device buffer of `nbytes` with a sentinel-filled guard before and behind it."""

    def __init__(self, nbytes, fill=0xA5):
        self.nbytes, self.fill = nbytes, fill
        self.raw = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def body(self, dtype):
        return self.raw[GUARD:GUARD + self.nbytes].view(dtype)

    def intact(self):
        return bool((self.raw[:GUARD] == self.fill).all()) and bool((self.raw[GUARD + self.nbytes:] == self.fill).all())


def run_label(mask, min_size):
    """c2s_label_components through the C ABI with guarded labels, count and workspace -> (labels, count, error word)."""
    from crop2seg_amd._lib import check, lib
    L = lib()
    nb, h, w = mask.shape
    md = torch.from_numpy(np.ascontiguousarray(mask)).cuda()
    need = L.c2s_label_components_workspace_bytes(nb, h, w)
    labels, count, ws = Guarded(4 * nb * h * w), Guarded(-(-4 * nb // 16) * 16), Guarded(need)
    assert ws.ptr() % 16 == 0
    err = torch.zeros(4, dtype=torch.int32, device="cuda")
    check(L.c2s_label_components(md.data_ptr(), labels.ptr(), count.ptr(), nb, h, w, min_size, ws.ptr(), need, err.data_ptr(),
                                 _stream()), "label_components")
    torch.cuda.synchronize()
    assert labels.intact() and count.intact() and ws.intact(), "a guard around labels / count / workspace was written"
    return labels.body(torch.int32).view(nb, h, w).cpu().numpy(), count.body(torch.int32)[:nb].cpu().numpy(), err.tolist()


@pytest.fixture(scope="module")
def reference_labels():
    return {name: PR.label_components(mask, ms) for name, (mask, ms) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_label_components(name, reference_labels):
    mask, min_size = CASES[name]
    labels, count, err = run_label(mask, min_size)
    want_labels, want_count = reference_labels[name]
    assert err == [0, 0, 0, 0]
    assert np.array_equal(count, want_count), (count, want_count)
    assert PR.same_labelling(labels, count, want_labels, want_count)
    again, count2, err2 = run_label(mask, min_size)
    assert np.array_equal(again, labels) and np.array_equal(count2, count) and err2 == [0, 0, 0, 0]    # bit-identical runs


def test_label_components_numbering_scan_over_many_workgroups():
    """B = 2, 301 x 299 random blobs.  PC_SCAN = 256 (csrc/parcels.hip) is the number of pixels one workgroup of the
    numbering scan covers: an image of 89999 pixels takes 352 such workgroups, and as 352 > 256 the scan over their sums
    (one workgroup of 256 lanes per image) also needs a second round with a carry."""
    mask = PR.random_blobs(2, 301, 299, seed=7)
    assert -(-301 * 299 // 256) > 256
    want_labels, want_count = PR.label_components(mask, PR.MIN_SIZE)
    assert want_count.min() > 50 and (want_labels == 0)[mask != 0].any()          # many parcels, and some small ones removed
    labels, count, err = run_label(mask, PR.MIN_SIZE)
    assert err == [0, 0, 0, 0] and np.array_equal(count, want_count)
    assert PR.same_labelling(labels, count, want_labels, want_count)
    again, count2, _ = run_label(mask, PR.MIN_SIZE)
    assert np.array_equal(again, labels) and np.array_equal(count2, count)
    one, cnt1, _ = run_label(mask, 1)                                              # min_size 1: every component numbered
    assert PR.same_labelling(one, cnt1, *PR.label_components(mask, 1))


def test_label_components_python_entry():
    from crop2seg_amd import postprocess as PP
    mask, min_size = CASES["touching"]
    labels, count = PP.label_components(torch.from_numpy(mask).cuda(), min_size)
    want_labels, want_count = PR.label_components(mask, min_size)
    assert labels.dtype == torch.int32 and PR.same_labelling(labels.cpu().numpy(), count.cpu().numpy(), want_labels, want_count)
    l2, c2 = PP.label_components(torch.from_numpy(mask[1]).cuda().bool(), min_size)          # [H,W] is B = 1; any dtype
    assert l2.shape == (PR.H, PR.W) and np.array_equal(l2.cpu().numpy(), want_labels[1]) and c2.tolist() == [want_count[1]]
    assert PP.check_errors() == (0, 0)


# ------------------------------------------------------------------------------------------------ seeds
@pytest.mark.parametrize("mode", ["probabilities", "logits", "separate_head", "separate_head_logits"])
def test_parcel_seeds(mode):
    """K = 16, boundary_code = 15; 2 x 37 x 53 pixels.  The generators discard every pixel whose top-2 probability lies
    within 1e-4 of the threshold or whose top two or three scores are closer than 1e-4 (and assert that none is left), so the
    float64 rule is unambiguous for the fp32 kernel."""
    from crop2seg_amd import postprocess as PP
    logits = mode.endswith("logits")
    thr = 0.3 if not mode.startswith("separate") else 0.7      # 0.7: both clauses of the separate-head rule decide pixels
    scores = PR.make_seed_scores(2, 16, PR.H, PR.W, seed=3, logits=logits)
    bscores = PR.make_boundary_scores(2, PR.H, PR.W, 4, thr, logits=logits) if mode.startswith("separate") else None
    want_mask, want_t1 = PR.seeds(scores, 15, thr, from_logits=logits, boundary_scores=bscores)
    assert 0.1 < want_mask.mean() < 0.9
    bd = torch.from_numpy(bscores).cuda() if bscores is not None else None
    mask = PP.parcel_seeds(torch.from_numpy(scores).cuda(), 15, thr, from_logits=logits, boundary_scores=bd)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), want_mask)
    m2, t1, _ = PP._seeds(torch.from_numpy(scores).cuda(), 15, thr, logits, bd, True)
    assert np.array_equal(m2.cpu().numpy(), want_mask) and np.array_equal(t1.cpu().numpy(), want_t1)
    if bscores is not None:                                    # boundary_code is ignored in this mode
        m3 = PP.parcel_seeds(torch.from_numpy(scores).cuda(), 3, thr, from_logits=logits, boundary_scores=bd)
        assert torch.equal(m3, mask)


def test_parcel_seeds_ties_go_to_the_lower_class():
    from crop2seg_amd import postprocess as PP
    p = np.zeros((1, 16, 1, 4), dtype=np.float32)
    p[0, [3, 15], 0, 0] = 0.5                   # 3 and 15 tie for the top: top-1 is 3, the boundary a strong second
    p[0, [0, 4], 0, 1] = 0.5                    # 0 and 4 tie: top-1 is the background
    p[0, 15, 0, 2], p[0, [2, 7], 0, 2] = 0.5, 0.25    # boundary first
    p[0, 5, 0, 3], p[0, [9, 15], 0, 3] = 0.5, 0.25    # 9 and 15 tie for the second place: the second is 9
    want_mask, want_t1 = PR.seeds(p, 15, 0.3, from_logits=False)
    assert want_mask.reshape(-1).tolist() == [0, 0, 0, 1] and want_t1.reshape(-1).tolist() == [3, 0, 15, 5]
    m, t1, _ = PP._seeds(torch.from_numpy(p).cuda(), 15, 0.3, False, None, True)
    assert np.array_equal(m.cpu().numpy(), want_mask) and np.array_equal(t1.cpu().numpy(), want_t1)


# ------------------------------------------------------------------------------------------------ vote
def vote_rasters():
    """K = 8, cap = 6, 2 x 12 x 16: hand-placed parcels (rows of 16 pixels)."""
    pred = np.full((2, 12, 16), 4, dtype=np.int64)
    labels = np.zeros((2, 12, 16), dtype=np.int32)
    labels[0, 0, :10], pred[0, 0, :5], pred[0, 0, 5:10] = 1, 3, 2          # parcel 1: classes 3 and 2 tie at 5: 2 wins
    labels[0, 1], pred[0, 1, :12], pred[0, 1, 12:] = 2, 0, 5               # parcel 2: background exactly 12 / 16 = 3/4
    labels[0, 2], pred[0, 2, :13], pred[0, 2, 13:] = 3, 0, 5               # parcel 3: one pixel above 3/4
    labels[0, 3, :7], pred[0, 3, :7] = 4, 0                                # parcel 4: background only
    labels[0, 5:9, 3:9], pred[0, 5:9, 3:9] = 6, 7                          # parcel 6; id 5 is carried by no pixel
    pred[0, 6, 4:8] = 1
    labels[0, 10, 0], labels[0, 10, 1] = 7, -2                             # labels outside [0, cap]
    pred[0, 11, 0], pred[0, 11, 5] = 8, -1                                 # classes outside [0, K): one without a parcel ...
    labels[0, 5, 3], pred[0, 5, 3] = 6, 9                                  # ... and one inside parcel 6
    rng = np.random.default_rng(2)
    labels[1] = rng.integers(0, 7, size=(12, 16))                          # image 1: the same ids, other parcels
    pred[1] = rng.integers(0, 8, size=(12, 16))
    return pred, labels


@pytest.mark.parametrize("bg_share", [0.75, None])
@pytest.mark.parametrize("outside", ["zero", "keep"])
def test_parcel_vote(bg_share, outside):
    from crop2seg_amd._lib import check, lib
    L = lib()
    K, cap, fill = 8, 6, -7
    pred, labels = vote_rasters()
    nb, h, w = pred.shape
    want_out, want_pc, want_hist, want_skipped, want_bad = PR.vote(pred, labels, K, cap, bg_share, outside, fill=fill)
    assert (want_skipped, want_bad) == (2, 3)
    assert want_pc[0].tolist() == ([2, 5, 0, 0, 0, 7] if bg_share is not None else [2, 5, 5, 0, 0, 7])
    need = L.c2s_parcel_vote_workspace_bytes(nb, cap, K)
    out, pc, hist = Guarded(8 * nb * h * w, fill=0xF9), Guarded(-(-4 * nb * cap // 16) * 16), Guarded(need)
    err = torch.zeros(4, dtype=torch.int32, device="cuda")
    pd, ld = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
    check(L.c2s_parcel_vote(pd.data_ptr(), ld.data_ptr(), out.ptr(), pc.ptr(), nb, h, w, K, cap,
                            -1.0 if bg_share is None else bg_share, 1 if outside == "keep" else 0, hist.ptr(), need,
                            err.data_ptr() + 4, _stream()), "parcel_vote")
    torch.cuda.synchronize()
    assert out.intact() and pc.intact() and hist.intact()
    assert err.tolist() == [0, want_skipped, want_bad, 0]
    got = out.body(torch.int64).view(nb, h, w).cpu().numpy()
    unwritten = np.frombuffer(b"\xf9" * 8, dtype=np.int64)[0]
    skipped = want_out == fill
    assert skipped.sum() == 5 and (got[skipped] == unwritten).all()                 # nothing is written for them
    assert np.array_equal(got[~skipped], want_out[~skipped])
    assert np.array_equal(pc.body(torch.int32)[:nb * cap].view(nb, cap).cpu().numpy(), want_pc)
    assert np.array_equal(hist.body(torch.int32).view(nb, cap, K).cpu().numpy(), want_hist)
    # the planted fault (>= at the background share) would have been rejected by the same comparisons
    if bg_share is not None:
        bad_out, bad_pc, _, _, _ = PR.vote(pred, labels, K, cap, bg_share, outside, ge=True, fill=fill)
        assert not np.array_equal(bad_pc, want_pc) and not np.array_equal(bad_out, want_out)


# ------------------------------------------------------------------------------------------------ chains and hooks
def lpis_like_parcels(nb, h, w, seed):
    """A rasterised parcel id map: the components of random blobs, numbered per image (0 = no parcel)."""
    return PR.label_components(PR.random_blobs(nb, h, w, seed, cell=7), 1)[0]


def test_homogenize_end_to_end():
    from crop2seg_amd import postprocess as PP
    rng = np.random.default_rng(12)
    parcels = lpis_like_parcels(2, 64, 64, 21)
    pred = np.repeat(np.repeat(rng.integers(0, 16, size=(2, 16, 16)), 4, 1), 4, 2)
    pred = np.where(rng.random((2, 64, 64)) < 0.55, 0, pred).astype(np.int64)        # much background: the share rule decides
    pd, ld = torch.from_numpy(pred).cuda(), torch.from_numpy(parcels).cuda()
    for bg_share, outside in ((0.75, "zero"), (0.75, "keep"), (0.25, "zero"), (None, "keep")):
        want = PR.homogenize(pred, parcels, 16, bg_share, outside)
        got = PP.homogenize(pd, ld, 16, bg_share, outside)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (bg_share, outside)
        small = PP.homogenize(pd, ld, 16, bg_share, outside, cap=int(parcels.max()))     # the table cut to the largest id
        assert torch.equal(small, got)
    one = PP.homogenize(pd[1], ld[1], 16)                                                # [H,W] is B = 1
    assert one.shape == (64, 64) and np.array_equal(one.cpu().numpy(), PR.homogenize(pred[1:], parcels[1:], 16)[0])
    assert PP.check_errors() == (0, 0)
    out, pc = PP.parcel_vote(pd, ld, 16, 0.75, "zero", cap=3)                             # ids above the cap are counted
    assert PP.check_errors() == (int((parcels > 3).sum()), 0)


def boundary_scene(logits, separate_head, thr):
    """2 x 16 x 64 x 64 scores: fields of 8 x 8 cells with one strong class each, lines of the boundary class (15) between
    them with a few gaps (so that some fields merge), noise from the seeds generator elsewhere; no borderline pixel.  With
    `separate_head` also the scores of a 2-class boundary head that draws the same lines."""
    rng = np.random.default_rng(34)
    ys, xs = np.mgrid[0:64, 0:64]
    ramp = (0.01 + 0.001 * np.arange(16))[None, :, None, None]              # the other classes: 1e-3 apart, no ties

    def strong(cls):
        p = np.zeros((2, 16, 64, 64))
        np.put_along_axis(p, cls[:, None], 0.8, 1)
        p = p + ramp
        p = p / p.sum(1, keepdims=True)
        return np.log(p) if logits else p

    field = np.repeat(np.repeat(rng.integers(0, 15, size=(2, 8, 8)), 8, 1), 8, 2)
    line = ((ys % 8 == 0) | (xs % 8 == 0))[None] & (rng.random((2, 64, 64)) < 0.93)
    inside = ~line & (rng.random((2, 64, 64)) < 0.9)
    scores = PR.make_seed_scores(2, 16, 64, 64, seed=31, logits=logits)
    scores = np.where(inside[:, None], strong(field), scores)
    if not separate_head:
        scores = np.where(line[:, None], strong(np.full((2, 64, 64), 15)), scores)
    scores = scores.astype(np.float32)
    assert not PR.borderline(PR.softmax64(scores, 1) if logits else scores.astype(np.float64), thr).any()
    if not separate_head:
        return scores, None
    bscores = PR.make_boundary_scores(2, 64, 64, 35, thr, logits=logits)
    sure = lambda p1: (np.log([1 - p1, p1]) if logits else np.array([1 - p1, p1]))[None, :, None, None]     # noqa: E731
    bscores = np.where(line[:, None], sure(0.9), np.where(inside[:, None], sure(0.05), bscores)).astype(np.float32)
    assert not PR.borderline_boundary(PR.softmax64(bscores, 1) if logits else bscores.astype(np.float64), thr).any()
    return scores, bscores


@pytest.mark.parametrize("mode", ["logits", "probabilities", "separate_head_logits"])
def test_homogenize_boundaries_end_to_end(mode):
    from crop2seg_amd import postprocess as PP
    logits = mode.endswith("logits")
    thr = 0.3
    scores, bscores = boundary_scene(logits, mode.startswith("separate"), thr)
    want = PR.homogenize_boundaries(scores, 15, thr, logits, bscores, PR.MIN_SIZE)
    assert len(np.unique(want)) > 6 and 0.3 < (want == 0).mean() < 0.9      # parcels of several classes survive, not all
    bd = torch.from_numpy(bscores).cuda() if bscores is not None else None
    got = PP.homogenize_boundaries(torch.from_numpy(scores).cuda(), 15, thr, logits, bd, PR.MIN_SIZE)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    assert PP.check_errors() == (0, 0)


def test_step_meters_with_parcels():
    """StepMeters.update(parcels=...): the IoU meter sees the homogenised top-1 prediction; the top-2 and the loss meter
    are what they are without parcels."""
    from crop2seg_amd.learning.metrics import StepMeters
    from oracle import tail_oracle as TO
    g = torch.Generator().manual_seed(41)
    K = 16
    logits = torch.randn(2, K, 64, 64, generator=g)
    logits[:, 0] += 1.5                                                       # enough background for the share rule to matter
    y = torch.randint(0, K, (2, 64, 64), generator=g)
    parcels = lpis_like_parcels(2, 64, 64, 43)
    plain, hooked = StepMeters(K, ignore_index=-1), StepMeters(K, ignore_index=-1)
    loss = torch.tensor([0.5], device="cuda")
    p0, p0_top2 = plain.update(logits.cuda(), y.cuda(), loss, want_pred=True)
    p1, p1_top2 = hooked.update(logits.cuda(), y.cuda(), loss, parcels=torch.from_numpy(parcels).cuda())
    want = PR.homogenize(logits.argmax(1).numpy(), parcels, K, 0.75, "zero")
    assert not np.array_equal(want, logits.argmax(1).numpy())
    assert np.array_equal(p1.cpu().numpy(), want) and torch.equal(p1_top2, p0_top2) and torch.equal(p0.cpu(), logits.argmax(1))
    assert np.array_equal(hooked.iou.conf_metric.conf.cpu().numpy(), TO.confusion_matrix(want, y.numpy(), K))
    assert torch.equal(hooked.iou_top2.conf_metric.conf, plain.iou_top2.conf_metric.conf)
    assert hooked.loss_mean() == plain.loss_mean() == 0.5
    hooked.update(logits.cuda(), y.cuda(), parcels=torch.from_numpy(parcels).cuda())                # the meter accumulates
    assert np.array_equal(hooked.iou.conf_metric.conf.cpu().numpy(), 2 * TO.confusion_matrix(want, y.numpy(), K))


def _predict_tile_before(model, x, dates, grid, crop, batch_size):
    """predict_tile as it was before the parcels hook: the same calls in the same order."""
    from crop2seg_amd import engine as E
    from crop2seg_amd._lib import check, lib
    n = x.shape[0]
    h1, w1 = x.shape[-2:]
    out_h, out_w = min(crop, grid * h1), min(crop, grid * w1)
    model.eval()
    proba = top1 = None
    with torch.no_grad():
        for first in range(0, n, batch_size):
            logits = model(x[first:first + batch_size].contiguous(), batch_positions=dates[first:first + batch_size].contiguous())
            K = logits.shape[1]
            if proba is None:
                proba = torch.empty(K, out_h, out_w, device=x.device, dtype=torch.float32)
                top1 = torch.empty(out_h, out_w, device=x.device, dtype=torch.int64)
            check(lib().c2s_softmax_stitch(logits.data_ptr(), proba.data_ptr(), top1.data_ptr(), first, logits.shape[0], K, h1, w1,
                                           grid, out_h, out_w, E._stream()), "softmax_stitch")
    model.check_health()
    return proba, top1


def test_predict_tile_with_parcels():
    """A 2 x 2 tile of 32 x 32 patches, cropped to 60 x 60, K = 16."""
    import crop2seg_amd as C2S
    from crop2seg_amd.inference import predict_tile
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=[32, 16])
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    net = net.cuda().eval()
    grid, h1, T, crop = 2, 32, 4, 60
    g = torch.Generator().manual_seed(19)
    x = torch.randn(grid * grid, T, 10, h1, h1, generator=g).cuda()
    dates = (5 * torch.arange(T))[None].repeat(grid * grid, 1).cuda()
    res = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4)
    assert isinstance(res, tuple) and len(res) == 2                        # today's calls: two tensors, bit for bit
    before = _predict_tile_before(net, x, dates, grid, crop, 4)
    assert torch.equal(res[0], before[0]) and torch.equal(res[1], before[1])
    proba, top1 = res
    # the boundary class: the second most frequent top-1 class of this seeded model, so that the rule has pixels to decide
    freq = np.bincount(top1.cpu().numpy().reshape(-1), minlength=16)
    code = int(np.argsort(-freq[1:], kind="stable")[1]) + 1
    p3, t3, hom = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4, boundary_homogenize=True, boundary_code=code)
    assert torch.equal(p3, proba) and torch.equal(t3, top1)
    want = PR.homogenize_boundaries(proba.cpu().numpy()[None], code, 0.3, False, None, PR.MIN_SIZE)[0]
    assert hom.shape == (crop, crop) and hom.dtype == torch.int64 and np.array_equal(hom.cpu().numpy(), want)
    parcels = lpis_like_parcels(1, crop, crop, 47)[0]
    p4, t4, hom4 = predict_tile(net, x, dates, grid=grid, crop=crop, batch_size=4, parcels=torch.from_numpy(parcels).cuda())
    assert torch.equal(p4, proba) and torch.equal(t4, top1)
    assert np.array_equal(hom4.cpu().numpy(), PR.homogenize(top1.cpu().numpy()[None], parcels[None], 16)[0])
    with pytest.raises(ValueError):
        predict_tile(net, x, dates, grid=grid, crop=crop, parcels=torch.from_numpy(parcels).cuda(), boundary_homogenize=True)
