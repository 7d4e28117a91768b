"""The yardstick of the parcel homogenisation (crop2seg_amd/postprocess.py, csrc/parcels.hip): a pure numpy / Python
restatement of the raster form of the reference's src/helpers/postprocess.py:377-604.

  * labelling: a two-pass union-find over the raster (4-connectivity, images independent), components under min_size removed,
    survivors numbered 1..n per image in raster order of their first pixel (= scipy.ndimage.label with the plus element when
    min_size = 1; tests/test_parcel_reference.py checks that where scipy imports);
  * seeds rule: in float64;
  * vote: Python integers, the background share compared as an exact fraction.

`connectivity=8`, `wrap=True` and `ge=True` are PLANTED FAULTS: wrong on purpose, so that the tests can show that their
comparisons reject them.  The mask patterns and generators below are shared by the CPU and the GPU tests.
"""
from fractions import Fraction

import numpy as np

B, H, W = 3, 37, 53             # no tile or wave boundary lines up with a row or an image
MIN_SIZE = 13                   # postprocess.py:557


# ------------------------------------------------------------------------------------------------ labelling
def label_components(mask, min_size=MIN_SIZE, connectivity=4, wrap=False):
    """mask [B,H,W] (non-zero = set) -> (labels int32 [B,H,W], count int32 [B])."""
    mask = np.asarray(mask) != 0
    nb, h, w = mask.shape
    labels = np.zeros((nb, h, w), dtype=np.int32)
    count = np.zeros(nb, dtype=np.int32)
    for b in range(nb):
        m = mask[b].reshape(-1).tolist()
        parent = list(range(h * w))

        def find(i):
            r = i
            while parent[r] != r:
                r = parent[r]
            while parent[i] != r:
                parent[i], i = r, parent[i]
            return r

        def unite(i, j):
            ri, rj = find(i), find(j)
            if ri < rj:
                parent[rj] = ri
            elif rj < ri:
                parent[ri] = rj

        for i in range(h * w):
            if not m[i]:
                continue
            x, y = i % w, i // w
            if (x > 0 or (wrap and i > 0)) and m[i - 1]:
                unite(i, i - 1)
            if y > 0 and m[i - w]:
                unite(i, i - w)
            if connectivity == 8 and y > 0:
                if x > 0 and m[i - w - 1]:
                    unite(i, i - w - 1)
                if x < w - 1 and m[i - w + 1]:
                    unite(i, i - w + 1)
        roots = [find(i) if m[i] else -1 for i in range(h * w)]
        sizes = {}
        for r in roots:
            if r >= 0:
                sizes[r] = sizes.get(r, 0) + 1
        ids = {r: n + 1 for n, r in enumerate(sorted(r for r, s in sizes.items() if s >= min_size))}
        labels[b] = np.array([ids.get(r, 0) for r in roots], dtype=np.int32).reshape(h, w)
        count[b] = len(ids)
    return labels, count


def _blob(canvas, b, y0, x0, n, width=4):
    """n pixels in rows of `width` from (y0, x0): one 4-connected component of exactly n pixels."""
    for k in range(n):
        canvas[b, y0 + k // width, x0 + k % width] = 1


def label_cases():
    """name -> (mask u8 [B,H,W], min_size)."""
    ys, xs = np.mgrid[0:H, 0:W]
    z = lambda: np.zeros((B, H, W), dtype=np.uint8)     # noqa: E731
    cases = {}
    cases["empty"] = (z(), MIN_SIZE)
    cases["full"] = (z() + 1, MIN_SIZE)
    serp = (ys % 2 == 0) | ((ys % 4 == 1) & (xs == W - 1)) | ((ys % 4 == 3) & (xs == 0))
    cases["serpentine"] = (np.broadcast_to(serp, (B, H, W)).astype(np.uint8), MIN_SIZE)     # one component, longest chains
    comb = (xs % 2 == 0) | (ys == H - 1)
    cases["comb"] = (np.broadcast_to(comb, (B, H, W)).astype(np.uint8), MIN_SIZE)           # teeth join in the last row only
    cases["checkerboard"] = (np.stack([(xs + ys + b) % 2 == 0 for b in range(B)]).astype(np.uint8), 1)
    cases["antidiagonal"] = (np.broadcast_to(xs + ys == H - 1, (B, H, W)).astype(np.uint8), 1)
    ring = (ys >= 5) & (ys <= 25) & (xs >= 5) & (xs <= 40) & ((ys == 5) | (ys == 25) | (xs == 5) | (xs == 40))
    island = (ys >= 12) & (ys <= 15) & (xs >= 20) & (xs <= 24)
    cases["ring"] = (np.broadcast_to(ring | island, (B, H, W)).astype(np.uint8), MIN_SIZE)
    blobs = z()
    for b in range(B):
        _blob(blobs, b, 2, 3 + b, MIN_SIZE - 1)         # removed
        _blob(blobs, b, 2, 20 + b, MIN_SIZE)            # kept
        _blob(blobs, b, 20, 30, MIN_SIZE - 1, width=1)  # a column of 12: removed
        _blob(blobs, b, 20, 40, MIN_SIZE, width=13)     # a row of 13: kept
    cases["blobs"] = (blobs, MIN_SIZE)
    touch = z()
    touch[0, H - 2:, 10:20] = 1                         # the last rows of image 0 ...
    touch[1, :2, 10:20] = 1                             # ... and the first rows of image 1, same columns: two components
    touch[2, 7:9, W - 7:] = 1                           # the end of rows 7 and 8 ...
    touch[2, 8:10, :7] = 1                              # ... and the start of rows 8 and 9: two components
    touch[1, 20, W - 13:] = 1                           # 13 pixels at the end of a row, and 13 at the start of the next:
    touch[1, 22, :13] = 1                               # (two rows apart: never one component)
    touch[0, 0, W - 7:] = 1                             # 7 + 6 pixels either side of a row end: a wrap would make them
    touch[0, 1, :6] = 1                                 # one component of 13, that is a survivor
    cases["touching"] = (touch, MIN_SIZE)
    return cases


def random_blobs(nb, h, w, seed, cell=9, p=0.62):
    """A mask of random blobs: coarse random cells with a ragged edge, like the interior of field parcels."""
    rng = np.random.default_rng(seed)
    coarse = rng.random((nb, -(-h // cell), -(-w // cell))) < p
    m = np.repeat(np.repeat(coarse, cell, 1), cell, 2)[:, :h, :w]
    m = m & (rng.random((nb, h, w)) < 0.93)
    m[:, ::cell, :] &= rng.random((nb, len(range(0, h, cell)), w)) < 0.35      # thin the cell borders: blobs come apart
    m[:, :, ::cell] &= rng.random((nb, h, len(range(0, w, cell)))) < 0.35
    return m.astype(np.uint8)


def same_labelling(got_labels, got_count, want_labels, want_count):
    """The comparison every labelling test uses: exact equality of the label raster and of the counts."""
    return np.array_equal(np.asarray(got_labels), want_labels) and np.array_equal(np.asarray(got_count), want_count)


# ------------------------------------------------------------------------------------------------ seeds
def softmax64(x, axis):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def seeds(scores, boundary_code=15, second_threshold=0.3, from_logits=True, boundary_scores=None):
    """scores [B,K,H,W] -> (mask u8 [B,H,W], t1 int64 [B,H,W]); float64 throughout, ties to the lower class."""
    p = softmax64(scores, 1) if from_logits else np.asarray(scores, dtype=np.float64)
    second_threshold = float(np.float32(second_threshold))      # the threshold as the float the kernel receives
    order = np.argsort(-p, axis=1, kind="stable")
    t1, t2 = order[:, 0], order[:, 1]
    p2 = np.take_along_axis(p, t2[:, None], 1)[:, 0]
    if boundary_scores is None:
        boundary = (t1 == boundary_code) | ((t2 == boundary_code) & (p2 > second_threshold))
    else:
        pb = softmax64(boundary_scores, 1) if from_logits else np.asarray(boundary_scores, dtype=np.float64)
        boundary = (pb[:, 1] >= pb[:, 0]) | (pb[:, 1] > second_threshold)
    return (~(boundary | (t1 == 0))).astype(np.uint8), t1.astype(np.int64)


def borderline(p, second_threshold, margin=1e-4):
    """Pixels of probabilities p [B,K,H,W] (float64) at which the seeds rule is within `margin` of flipping: the top-2
    probability near the threshold, or two of the three largest scores close to each other."""
    s = -np.sort(-p, axis=1)
    return (np.abs(s[:, 1] - second_threshold) < margin) | (s[:, 0] - s[:, 1] < margin) | (s[:, 1] - s[:, 2] < margin)


def borderline_boundary(pb, second_threshold, margin=1e-4):
    return (np.abs(pb[:, 1] - pb[:, 0]) < 2 * margin) | (np.abs(pb[:, 1] - second_threshold) < margin)


def make_seed_scores(nb, k, h, w, seed, boundary_code=15, second_threshold=0.3, logits=False):
    """float32 class scores [nb,k,h,w] (probabilities, or logits of them) without a borderline pixel; every branch of the
    rule occurs: boundary first, boundary a strong / a weak second, class 0 first, plain seeds."""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(k, 0.35), size=(nb, h, w)).transpose(0, 3, 1, 2)
    # make the boundary class the runner-up on about a third of the pixels, with a share on either side of the threshold
    pick = rng.random((nb, h, w)) < 0.35
    share = rng.uniform(second_threshold - 0.15, second_threshold + 0.15, size=(nb, h, w))
    rest = p.copy()
    rest[:, boundary_code] = 0
    rest = rest / rest.sum(1, keepdims=True) * (1 - share)[:, None]
    rest[:, boundary_code] = share
    p = np.where(pick[:, None], rest, p)
    if logits:
        scores = (np.log(np.maximum(p, 1e-30)) + rng.uniform(-3, 3, size=(nb, 1, h, w))).astype(np.float32)
        seen = softmax64(scores, 1)
    else:
        scores = p.astype(np.float32)
        seen = scores.astype(np.float64)
    bad = borderline(seen, second_threshold)
    safe = np.full(k, 0.02 / (k - 2))                  # a pixel far from every decision: class 1 at 0.9, class 2 at 0.08
    safe[1], safe[2] = 0.9, 0.08
    fill = (np.log(safe) if logits else safe).astype(np.float32)
    scores = np.where(bad[:, None], fill[None, :, None, None], scores)
    seen = softmax64(scores, 1) if logits else scores.astype(np.float64)
    assert not borderline(seen, second_threshold).any(), "a borderline pixel is left"
    return np.ascontiguousarray(scores)


def make_boundary_scores(nb, h, w, seed, second_threshold, logits=False):
    """float32 scores of a 2-class boundary head [nb,2,h,w] without a borderline pixel."""
    rng = np.random.default_rng(seed)
    p1 = rng.random((nb, h, w))
    p = np.stack([1 - p1, p1], 1)
    if logits:
        scores = (np.log(np.maximum(p, 1e-30)) + rng.uniform(-2, 2, size=(nb, 1, h, w))).astype(np.float32)
        seen = softmax64(scores, 1)
    else:
        scores = p.astype(np.float32)
        seen = scores.astype(np.float64)
    bad = borderline_boundary(seen, second_threshold)
    fill = (np.log([0.9, 0.1]) if logits else np.array([0.9, 0.1])).astype(np.float32)
    scores = np.where(bad[:, None], fill[None, :, None, None], scores)
    seen = softmax64(scores, 1) if logits else scores.astype(np.float64)
    assert not borderline_boundary(seen, second_threshold).any(), "a borderline pixel is left"
    return np.ascontiguousarray(scores)


# ------------------------------------------------------------------------------------------------ vote
def vote_rule(counts, bg_share, ge=False):
    """The winner of one parcel from its per-class pixel counts (Python ints).  bg_share None: class 0 is never a candidate."""
    counts = [int(c) for c in counts]
    total = sum(counts)
    best, win = 0, 0
    if bg_share is not None and bg_share >= 0 and counts[0] > 0:
        bound = Fraction(float(np.float32(bg_share))) * total           # the share as the float the kernel receives
        if (Fraction(counts[0]) >= bound) if ge else (Fraction(counts[0]) > bound):
            best = counts[0]
    for k in range(1, len(counts)):
        if counts[k] > best:
            best, win = counts[k], k
    return win


def vote(pred, labels, num_classes, cap, bg_share=None, outside="zero", ge=False, fill=None):
    """-> (out int64 [B,H,W], parcel_class int32 [B,cap], hist int32 [B,cap,K], skipped labels, bad classes).
    Pixels with a label outside [0,cap] or a class outside [0,K) are counted and left as `fill` in out."""
    pred, labels = np.asarray(pred, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    nb = pred.shape[0]
    k = num_classes
    bad_label = (labels < 0) | (labels > cap)
    bad_class = (pred < 0) | (pred >= k)
    live = (labels > 0) & ~bad_label & ~bad_class
    hist = np.zeros((nb, cap, k), dtype=np.int32)
    for b in range(nb):
        np.add.at(hist[b], (labels[b][live[b]] - 1, pred[b][live[b]]), 1)
    parcel_class = np.array([[vote_rule(hist[b, p].tolist(), bg_share, ge) for p in range(cap)] for b in range(nb)],
                            dtype=np.int32).reshape(nb, cap)
    out = np.where(outside == "keep", pred, 0).astype(np.int64)
    out = np.broadcast_to(out, pred.shape).copy()
    for b in range(nb):
        out[b][live[b]] = parcel_class[b][labels[b][live[b]] - 1]
    skip = bad_label | bad_class
    if skip.any():
        assert fill is not None
        out[skip] = np.broadcast_to(np.asarray(fill), out.shape)[skip]
    return out, parcel_class, hist, int(bad_label.sum()), int(bad_class.sum())


def vote_cap(h, w, min_size):
    return h * w // min_size + 1


def homogenize(pred, parcels, num_classes, bg_share=0.75, outside="zero"):
    cap = max(1, int(np.asarray(parcels).max()))
    return vote(pred, parcels, num_classes, cap, bg_share, outside)[0]


def homogenize_boundaries(scores, boundary_code=15, second_threshold=0.3, from_logits=True, boundary_scores=None,
                          min_size=MIN_SIZE):
    mask, t1 = seeds(scores, boundary_code, second_threshold, from_logits, boundary_scores)
    labels, _ = label_components(mask, min_size)
    k = np.asarray(scores).shape[1]
    return vote(t1, labels, k, vote_cap(mask.shape[1], mask.shape[2], min_size), None, "zero")[0]
