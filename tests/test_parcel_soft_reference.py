"""CPU checks of tests/parcel_soft_ref.py, the yardstick of the soft parcel vote: the integer restatement against a plain
per-parcel loop that follows the reference's `soften` (src/helpers/postprocess.py:238-281) step by step, the planted faults,
and the argument validation of the Python entry points (which needs no device)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parcel_soft_ref as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def soften_loop(p, labels, cap, bg_mean=0.7):
    """`soften` on rasters: per polygon the float64 mean of every class column over the points it covers (groupby.mean),
    torch.topk(k=2) over the table, and where top1 is 0 the replacement `mean > 0.7 ? 0 : top2`."""
    nb, k = p.shape[:2]
    label = np.zeros((nb, cap), dtype=np.int32)
    top2 = np.zeros((nb, cap), dtype=np.int32)
    mean = np.zeros((nb, cap, k), dtype=np.float64)
    for b in range(nb):
        for i in range(cap):
            points = labels[b] == i + 1
            if not points.any():
                continue
            vals = np.stack([p[b, c][points].astype(np.float64).mean() for c in range(k)])
            top = torch.from_numpy(vals[None]).topk(k=2, dim=1)
            t1, t2 = int(top[1][0, 0]), int(top[1][0, 1])
            if t1 == 0:
                t1 = 0 if float(top[0][0, 0]) > bg_mean else t2
            label[b, i], top2[b, i], mean[b, i] = t1, t2, vals
    return label, top2, mean


@pytest.fixture(scope="module")
def scenes():
    return {k: SR.make_soft_scene(2, k, 40, 72, seed=50 + k) for k in (2, 15, 16, 32)}


@pytest.mark.parametrize("k", [2, 15, 16, 32])
def test_integer_restatement_equals_the_soften_loop(k, scenes):
    """Labels and top-2 exactly; means within 2e-8 + 2^-24 * mean: the quantisation moves a pixel's probability, hence a
    mean, by at most 2^-33 (1.2e-10), the double division and the one rounding to float add 2^-24 relative."""
    p, labels, cap = scenes[k]
    got = SR.soft_vote(p, labels, cap)
    label, top2, mean = soften_loop(p, labels, cap)
    used = got["pixels"] > 0
    assert used.sum() > 10 and (~used).any() and (labels == 0).any()
    if k > 2:
        led = (got["top2"] != got["label"]) & used                          # background-led parcels on both sides of 0.7
        assert (led & (got["label"] == 0)).any() and (used & (got["label"] == got["top2"])).any()
    assert np.array_equal(got["label"], label) and np.array_equal(got["top2"], top2)
    err = np.abs(got["mean"].astype(np.float64) - mean)
    print(f"K = {k}: max |mean - float64 mean| = {err.max():.3e}")
    assert (err <= 2e-8 + 2.0 ** -24 * mean).all()
    f64 = SR.soft_vote64(p, labels, cap, from_logits=False)
    assert np.array_equal(f64["label"], label) and np.array_equal(f64["top2"], top2) and np.array_equal(f64["out"], got["out"])
    assert np.array_equal(f64["pixels"], got["pixels"])


def edge_scene():
    """K = 4, one image of 6 rows of 16 pixels, a parcel per row, probabilities exactly representable: the inputs at which
    each planted fault shows."""
    p = np.zeros((1, 4, 6, 16), dtype=np.float32)
    labels = np.repeat(np.arange(1, 7, dtype=np.int32)[None, :, None], 16, 2)
    p[0, 1, 0], p[0, 2, 0] = 0.5, 0.5                      # 1: classes 1 and 2 tie: the lower first
    p[0, 0, 1], p[0, 1, 1] = 0.75, 0.25                    # 2: the background exactly at bg_mean = 0.75: not above it
    p[0, 0, 2], p[0, 1, 2] = 0.75, 0.25                    # 3: one pixel above: the background keeps the parcel
    p[0, 0, 2, 5], p[0, 1, 2, 5] = 0.875, 0.125
    p[0, 3, 3] = 1.0                                       # 4: q(1.0) = 2^32 does not fit 32 bits
    p[0, 0, 4], p[0, 2, 4], p[0, 3, 4] = 0.5, 0.25, 0.25   # 5: background-led and below: top2 stays 2, the label is 2
    p[0, 0, 5], p[0, 3, 5] = 0.25, 0.75                    # 6: nothing special
    return p, labels, 6


def test_rule_edges_of_the_restatement():
    p, labels, cap = edge_scene()
    got = SR.soft_vote(p, labels, cap, bg_mean=0.75)
    assert got["label"][0].tolist() == [1, 1, 0, 3, 2, 3]
    assert got["top2"][0].tolist() == [2, 1, 1, 0, 2, 0]
    assert got["pixels"][0].tolist() == [16] * 6
    assert got["mean"][0, 3].tolist() == [0, 0, 0, 1.0] and int(got["sums"][0, 3, 3]) == 16 << 32
    assert np.array_equal(got["out"][0], np.repeat(np.array([1, 1, 0, 3, 2, 3])[:, None], 16, 1))


@pytest.mark.parametrize("fault", ["ge", "q32", "ties_high", "top2_follows"])
def test_planted_faults_are_rejected(fault):
    p, labels, cap = edge_scene()
    want = SR.soft_vote(p, labels, cap, bg_mean=0.75)
    bad = SR.soft_vote(p, labels, cap, bg_mean=0.75, **{fault: True})
    assert SR.same_table(want, SR.soft_vote(p, labels, cap, bg_mean=0.75))
    assert not SR.same_table(bad, want)
    row = {"ge": 1, "q32": 3, "ties_high": 0, "top2_follows": 4}[fault]     # and it shows where it was planted
    field = {"ge": "label", "q32": "mean", "ties_high": "label", "top2_follows": "top2"}[fault]
    assert not np.array_equal(bad[field][0, row], want[field][0, row])


def test_quantisation_rounds_halves_to_even_and_clamps():
    q = SR.quantise(np.array([1.5 * 2.0 ** -32, 2.5 * 2.0 ** -32, 1.0, 1.5, -0.25, np.float32(0.7)], dtype=np.float32))
    assert q.tolist() == [2, 2, 1 << 32, 1 << 32, 0, int(float(np.float32(0.7)) * 2 ** 32)]


def test_scene_generator_leaves_no_borderline_parcel():
    for logits in (False, True):
        scores, labels, cap = SR.make_soft_scene(2, 16, 48, 52, seed=9, logits=logits)
        seen = SR.PR.softmax64(scores, 1) if logits else scores.astype(np.float64)
        m, n = SR.mean_table(seen, labels, cap)
        assert not SR.borderline_parcels(m, n).any() and scores.dtype == np.float32
        used = np.unique(labels[labels > 0])
        assert len(used) < cap and set(range(1, cap + 1)) - set(used.tolist())          # gaps in the id range


# ------------------------------------------------------------------------------------------------ validation, no device
def test_parcel_soft_vote_validates_before_any_device():
    from crop2seg_amd import postprocess as PP
    s, l = torch.zeros(1, 4, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int32)
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(s, l, outside="nowhere")
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(s, l, bg_mean=float("nan"))
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(s, l, bg_mean=None)
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(s, l, cap=0)
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(s, torch.zeros(1, 8, 9, dtype=torch.int32))
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(torch.zeros(1, 33, 8, 8), l)
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(torch.zeros(1, 1, 8, 8), l)
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(torch.zeros(8, 8), torch.zeros(8, 8))
    with pytest.raises(ValueError):
        PP.parcel_soft_vote(torch.zeros(1, 4, 8, 8, dtype=torch.int64), l)
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # valid arguments: only the device is missing
        PP.parcel_soft_vote(s, l)


def test_homogenize_type_is_validated():
    from crop2seg_amd import postprocess as PP
    s, l = torch.zeros(1, 4, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int32)
    with pytest.raises(ValueError):
        PP.homogenize(s, l, 4, type_="medium")
    with pytest.raises(ValueError):
        PP.homogenize(s, l, 5, type_="soft")                                # K of the scores is not num_classes
    with pytest.raises(ValueError):
        PP.homogenize(s, l, 4, type_="soft", bg_mean=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.homogenize(s, l, 4, type_="soft")


def test_predict_entries_validate_parcel_mode():
    from crop2seg_amd.inference import predict_raster, predict_tile
    from crop2seg_amd.learning.metrics import StepMeters
    series, dates = torch.zeros(2, 10, 40, 40), torch.zeros(2, dtype=torch.int64)
    for kw in (dict(parcel_mode="mean"), dict(parcel_cap=0), dict(parcel_cap=2.5)):
        with pytest.raises(ValueError):
            predict_raster(None, series, dates, patch=32, stride=24, **kw)
        with pytest.raises(ValueError):
            predict_tile(None, torch.zeros(4, 2, 10, 32, 32), torch.zeros(4, 2), grid=2, crop=60, **kw)
    with pytest.raises(ValueError):
        StepMeters(4, device="cpu").update(torch.zeros(1, 4, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64), parcel_mode="mean")


def test_soft_vote_is_declared_in_signatures_and_header():
    from crop2seg_amd import _lib
    header = open(os.path.join(ROOT, "include", "c2s_hip.h")).read()
    for name, nargs in (("c2s_parcel_soft_vote_workspace_bytes", 3), ("c2s_parcel_soft_vote", 19)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        proto = re.search(r"\b" + name + r"\(([^)]*)\);", header)
        assert proto and len(proto.group(1).split(",")) == nargs
    assert "postprocess.py:238-281" in header
