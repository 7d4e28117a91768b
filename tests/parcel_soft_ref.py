"""The yardstick of the soft parcel vote (crop2seg_amd/postprocess.py `parcel_soft_vote`, csrc/parcels.hip): restatements of
the raster form of the reference's `soften` (src/helpers/postprocess.py:238-281) and of the rasterisation of its `soft_label`
(:491-507).

  * `soft_vote`: the integer restatement.  Probabilities are quantised to 2^-32 fixed point in numpy uint64, summed per
    parcel, and the rule runs on Python ints; the background compare and the means go through doubles exactly as the kernel
    states them (include/c2s_hip.h).  A kernel that keeps the contract matches it bit for bit.
  * `soft_vote64`: the float64 restatement (softmax via parcel_ref.softmax64): the yardstick under from_logits, where the
    kernel's fp32 softmax is not reproduced bit for bit.
  * `make_soft_scene`: scenes without a borderline parcel, shared by the CPU and the GPU tests.

`ge=True`, `q32=True`, `ties_high=True` and `top2_follows=True` are PLANTED FAULTS: wrong on purpose, so that the tests can
show that their comparisons reject them.
"""
import numpy as np

import parcel_ref as PR

BG_MEAN = 0.7                   # postprocess.py:273
MARGIN = 1e-4                   # parcel_ref.borderline's margin
TWO32 = 4294967296.0


# ------------------------------------------------------------------------------------------------ integer restatement
def quantise(p, q32=False):
    """q(p) = rint(clamp(p, 0, 1) * 2^32) as uint64 (numpy's rint rounds halves to even, as the kernel's)."""
    q = np.rint(np.clip(np.asarray(p, dtype=np.float64), 0.0, 1.0) * TWO32).astype(np.uint64)
    if q32:
        q = q & np.uint64(0xFFFFFFFF)                                       # PLANTED: q(1.0) = 2^32 wraps to 0
    return q


def soft_rule(sums, n, bg_mean=BG_MEAN, ge=False, ties_high=False, top2_follows=False):
    """One parcel: sums = the K fixed-point sums (Python ints), n > 0 its pixels -> (label, top2)."""
    sums = [int(s) for s in sums]
    order = sorted(range(len(sums)), key=lambda k: (-sums[k], -k if ties_high else k))
    t1, t2 = order[0], order[1]
    label, top2 = t1, t2
    if t1 == 0:
        lhs = float(sums[0])                                                # (double)S_0: round to nearest even
        rhs = float(np.float32(bg_mean)) * float(n) * TWO32                 # the float the kernel receives, in doubles
        if not ((lhs >= rhs) if ge else (lhs > rhs)):
            label = t2
            if top2_follows:
                top2 = order[2] if len(sums) > 2 else t1                    # PLANTED: the runner-up moves on as well
    return label, top2


def _top1(p):
    """First maximum per pixel, a NaN counting as the largest value (as the kernels compare)."""
    return np.argmax(np.where(np.isnan(p), np.inf, p), axis=1).astype(np.int64)


def soft_vote(p, labels, cap, bg_mean=BG_MEAN, outside="zero", fill=None, ge=False, q32=False, ties_high=False,
              top2_follows=False):
    """p f32 probabilities [B,K,H,W], labels [B,H,W] -> dict(out int64 [B,H,W], label / top2 / pixels int32 [B,cap],
    mean f32 [B,cap,K], sums uint64 [B,cap,K], skipped = labels outside [0,cap], nonfinite = parcel pixels left out for a
    NaN or infinite score).  Skipped pixels are left as `fill` in out."""
    p = np.asarray(p, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    nb, k, h, w = p.shape
    bad_label = (labels < 0) | (labels > cap)
    inside = (labels > 0) & ~bad_label
    finite = np.isfinite(p).all(axis=1)
    live = inside & finite
    q = quantise(np.where(np.isfinite(p), p, 0), q32)
    sums = np.zeros((nb, cap, k), dtype=np.uint64)
    pixels = np.zeros((nb, cap), dtype=np.int32)
    for b in range(nb):
        idx = labels[b][live[b]] - 1
        np.add.at(pixels[b], idx, 1)
        np.add.at(sums[b], idx, q[b][:, live[b]].T)
    label = np.zeros((nb, cap), dtype=np.int32)
    top2 = np.zeros((nb, cap), dtype=np.int32)
    mean = np.zeros((nb, cap, k), dtype=np.float32)
    for b in range(nb):
        for i in range(cap):
            n = int(pixels[b, i])
            if n == 0:
                continue
            s = [int(x) for x in sums[b, i]]
            label[b, i], top2[b, i] = soft_rule(s, n, bg_mean, ge, ties_high, top2_follows)
            mean[b, i] = [np.float32(float(x) / (float(n) * TWO32)) for x in s]
    out = _top1(p) if outside == "keep" else np.zeros((nb, h, w), dtype=np.int64)
    for b in range(nb):
        out[b][inside[b]] = label[b][labels[b][inside[b]] - 1]
    if bad_label.any():
        assert fill is not None
        out[bad_label] = fill
    return dict(out=out, label=label, top2=top2, mean=mean, pixels=pixels, sums=sums, skipped=int(bad_label.sum()),
                nonfinite=int((inside & ~finite).sum()))


# ------------------------------------------------------------------------------------------------ float64 restatement
def mean_table(p64, labels, cap):
    """float64 means [B,cap,K] and pixel counts [B,cap] of probabilities p64 [B,K,H,W] over the parcels (all finite)."""
    labels = np.asarray(labels, dtype=np.int64)
    nb, k = p64.shape[:2]
    live = (labels > 0) & (labels <= cap)
    tot = np.zeros((nb, cap, k), dtype=np.float64)
    n = np.zeros((nb, cap), dtype=np.int64)
    for b in range(nb):
        idx = labels[b][live[b]] - 1
        np.add.at(n[b], idx, 1)
        np.add.at(tot[b], idx, p64[b][:, live[b]].T)
    return tot / np.maximum(n, 1)[..., None], n


def soft_vote64(scores, labels, cap, bg_mean=BG_MEAN, outside="zero", from_logits=True):
    """float64 throughout; ties to the lower class.  -> dict(out, label, top2, mean float64, pixels)."""
    p = PR.softmax64(scores, 1) if from_logits else np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    m, n = mean_table(p, labels, cap)
    order = np.argsort(-m, axis=2, kind="stable")
    t1, t2 = order[..., 0], order[..., 1]
    bg = m[..., 0] > float(np.float32(bg_mean))
    label = np.where((t1 == 0) & ~bg, t2, t1)
    label, t2 = np.where(n > 0, label, 0).astype(np.int32), np.where(n > 0, t2, 0).astype(np.int32)
    out = _top1(p) if outside == "keep" else np.zeros(labels.shape, dtype=np.int64)
    inside = (labels > 0) & (labels <= cap)
    for b in range(labels.shape[0]):
        out[b][inside[b]] = label[b][labels[b][inside[b]] - 1]
    return dict(out=out, label=label, top2=t2, mean=m * (n > 0)[..., None], pixels=n.astype(np.int32))


# ------------------------------------------------------------------------------------------------ scenes
def borderline_parcels(m, n, bg_mean=BG_MEAN, margin=MARGIN):
    """[B,cap] bool: parcels (n > 0) whose float64 means m [B,cap,K] are within `margin` of flipping a decision: the two
    or three largest means close to each other, or the background mean near bg_mean."""
    s = -np.sort(-m, axis=2)
    bad = (s[..., 0] - s[..., 1] < margin) | (np.abs(m[..., 0] - float(np.float32(bg_mean))) < margin)
    if m.shape[2] > 2:
        bad |= s[..., 1] - s[..., 2] < margin
    return bad & (n > 0)


def irregular_parcels(nb, h, w, seed):
    """int32 [nb,h,w] parcel ids with gaps in the id range (every fourth id and the last two are carried by no pixel),
    label-0 pixels between the parcels, and parcels of several pieces (every seventh component joins its predecessor)
    -> (labels, cap)."""
    comp, count = PR.label_components(PR.random_blobs(nb, h, w, seed, cell=5, p=0.5), 1)
    comp = comp.astype(np.int64)
    comp = np.where((comp > 1) & (comp % 7 == 0), comp - 1, comp)
    labels = np.where(comp > 0, comp + (comp - 1) // 3, 0).astype(np.int32)
    return labels, int(labels.max()) + 2


def make_soft_scene(nb, k, h, w, seed, bg_mean=BG_MEAN, logits=False, labels=None, cap=None):
    """-> (scores f32 [nb,k,h,w], labels int32 [nb,h,w], cap): Dirichlet scores pulled towards one class per parcel; about
    a fifth of the parcels are led by the background, with a mean on either side of bg_mean.  Every borderline parcel is
    overwritten with a safe distribution, and none is left (asserted)."""
    rng = np.random.default_rng(seed)
    if labels is None:
        labels, cap = irregular_parcels(nb, h, w, seed + 1000)
    labels = np.asarray(labels, dtype=np.int32)
    p = rng.dirichlet(np.full(k, 0.35), size=(nb, h, w)).transpose(0, 3, 1, 2)
    lead = rng.integers(1, k, size=(nb, cap + 1))                           # per parcel: the class it is pulled towards
    pull = rng.uniform(0.15, 0.6, size=(nb, cap + 1))
    bg_led = rng.random((nb, cap + 1)) < 0.2
    target = np.where(rng.random((nb, cap + 1)) < 0.5, bg_mean - 0.1, bg_mean + 0.1)      # the background mean aimed at
    lead = np.where(bg_led, 0, lead)
    pull = np.where(bg_led, (target - 1.0 / k) / (1.0 - 1.0 / k), pull)
    pull[:, 0] = 0                                                          # pixels without a parcel: plain Dirichlet
    lab = np.clip(labels, 0, cap)
    bi = np.arange(nb)[:, None, None]
    a = (pull[bi, lab] * rng.uniform(0.8, 1.2, size=(nb, h, w))).clip(0, 0.95)
    onehot = np.zeros((nb, k, h, w))
    np.put_along_axis(onehot, lead[bi, lab][:, None], 1.0, 1)
    p = a[:, None] * onehot + (1 - a[:, None]) * p

    def as_scores(q):
        if logits:
            return (np.log(np.maximum(q, 1e-30)) + rng.uniform(-3, 3, size=(nb, 1, h, w))).astype(np.float32)
        return q.astype(np.float32)

    def seen(s):
        return PR.softmax64(s, 1) if logits else s.astype(np.float64)

    scores = as_scores(p)
    bad = borderline_parcels(*mean_table(seen(scores), labels, cap), bg_mean)
    safe = np.full(k, 0.02 / max(k - 2, 1))            # far from every decision: class 1 at 0.9, class 2 at 0.08
    safe[1] = 0.9
    if k > 2:
        safe[2] = 0.08
    else:
        safe[0] = 0.1
    hit = np.concatenate([np.zeros((nb, 1), bool), bad], 1)[bi, lab]
    scores = np.where(hit[:, None], as_scores(np.broadcast_to(safe[None, :, None, None], p.shape)), scores)
    m, n = mean_table(seen(scores), labels, cap)
    assert not borderline_parcels(m, n, bg_mean).any(), "a borderline parcel is left"
    return np.ascontiguousarray(scores), labels, cap


def same_table(got, want, fields=("out", "label", "top2", "pixels", "mean")):
    """The comparison the bit-for-bit tests use: exact equality of every field (means as their bit patterns)."""
    for f in fields:
        g, w_ = np.asarray(got[f]), np.asarray(want[f])
        if f == "mean":
            g, w_ = g.astype(np.float32).view(np.uint32), w_.astype(np.float32).view(np.uint32)
        if g.shape != w_.shape or not np.array_equal(g, w_):
            return False
    return True
