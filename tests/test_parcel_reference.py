"""CPU checks of the parcel homogenisation's yardstick (tests/parcel_ref.py) and of the C ABI's argument checks: the
restatement against scipy.ndimage.label where scipy imports, planted faults that the GPU test's comparisons must reject,
the vote rule on hand-written histograms, and the refusals of the entry points (no GPU needed: they return before a launch)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parcel_ref as PR  # noqa: E402

CASES = PR.label_cases()


@pytest.fixture(scope="module")
def reference_labels():
    return {name: PR.label_components(mask, ms) for name, (mask, ms) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_scipy_label(name, reference_labels):
    """min_size = 1: scipy's numbering exactly; the cases' own min_size: scipy's components minus the small ones, renumbered."""
    ndi = pytest.importorskip("scipy.ndimage")
    mask, min_size = CASES[name]
    plus = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    one, cnt = PR.label_components(mask, 1)
    got, got_cnt = reference_labels[name]
    for b in range(mask.shape[0]):
        lab, n = ndi.label(mask[b], plus)
        assert n == cnt[b] and np.array_equal(lab, one[b])
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
        keep = np.array([0] + [1 if sizes[i] >= min_size else 0 for i in range(1, n + 1)])
        renum = np.cumsum(keep) * keep
        assert np.array_equal(renum[lab], got[b]) and got_cnt[b] == keep.sum()


def test_cases_hold_what_they_are_for(reference_labels):
    n = PR.H * PR.W
    assert reference_labels["empty"][1].tolist() == [0, 0, 0] and reference_labels["full"][1].tolist() == [1, 1, 1]
    assert reference_labels["serpentine"][1].tolist() == [1, 1, 1] and reference_labels["comb"][1].tolist() == [1, 1, 1]
    assert reference_labels["checkerboard"][1].tolist() == [(n + 1) // 2, n // 2, (n + 1) // 2]
    assert reference_labels["antidiagonal"][1].tolist() == [PR.H] * 3
    assert reference_labels["ring"][1].tolist() == [2, 2, 2]
    assert reference_labels["blobs"][1].tolist() == [2, 2, 2]                 # the two of min_size - 1 pixels are removed
    assert int(PR.label_components(CASES["blobs"][0], PR.MIN_SIZE - 1)[1][0]) == 4
    assert reference_labels["touching"][1].tolist() == [1, 3, 2]


def test_planted_faults_are_rejected(reference_labels):
    """The comparison of the GPU test (PR.same_labelling) fails for 8-connectivity and for a row wrap-around."""
    def rejected(fault, names):
        return [name for name in names
                if not PR.same_labelling(*PR.label_components(CASES[name][0], CASES[name][1], **fault), *reference_labels[name])]

    assert set(rejected(dict(connectivity=8), CASES)) >= {"checkerboard", "antidiagonal"}
    assert "touching" in rejected(dict(wrap=True), CASES)
    # a leak between images: label the batch as one tall image
    mask, ms = CASES["touching"]
    tall, cnt = PR.label_components(mask.reshape(1, -1, PR.W), ms)
    assert not PR.same_labelling(tall.reshape(mask.shape), cnt, *reference_labels["touching"])
    assert int(cnt[0]) == 5                                                   # the two blocks across the image edge are one


def test_vote_rule_on_handwritten_histograms():
    assert PR.vote_rule([75, 25, 0, 0], 0.75) == 1            # exactly 3/4 background: not a candidate
    assert PR.vote_rule([76, 24, 0, 0], 0.75) == 0            # one pixel above
    assert PR.vote_rule([75, 25, 0, 0], 0.75, ge=True) == 0   # the planted fault differs exactly here
    assert PR.vote_rule([3, 1, 0, 0], 0.75) == 1 and PR.vote_rule([3, 0, 0, 0], 0.75) == 0
    assert PR.vote_rule([0, 5, 5, 1], 0.75) == 1              # ties go to the lower class
    assert PR.vote_rule([0, 2, 7, 7], None) == 2
    assert PR.vote_rule([80, 10, 10, 0], 0.75) == 0
    assert PR.vote_rule([9, 0, 0, 0], None) == 0              # background only, no candidate: 0
    assert PR.vote_rule([0, 0, 0, 0], 0.75) == 0              # an id no pixel carries
    assert PR.vote_rule([90, 0, 0, 10], None) == 3            # raster_val > 0: background never wins a boundary parcel
    assert PR.vote_rule([10, 10, 0, 0], 0.25) == 0            # background a candidate and tied: the lower class


def test_vote_planted_fault_is_rejected_by_the_raster_comparison():
    pred = np.zeros((1, 4, 4), dtype=np.int64)
    pred[0, 0] = 2                                             # 12 of 16 pixels background: exactly 3/4
    labels = np.ones((1, 4, 4), dtype=np.int32)
    out, pc, hist, _, _ = PR.vote(pred, labels, 4, 1, 0.75)
    bad, pc_bad, _, _, _ = PR.vote(pred, labels, 4, 1, 0.75, ge=True)
    assert hist[0, 0].tolist() == [12, 0, 4, 0] and pc.tolist() == [[2]] and (out == 2).all()
    assert not np.array_equal(out, bad) and pc_bad.tolist() == [[0]]


def test_seed_generators_leave_no_borderline_pixel():
    for logits in (False, True):
        s = PR.make_seed_scores(2, 16, 16, 16, 5, logits=logits)
        mask, t1 = PR.seeds(s, 15, 0.3, from_logits=logits)
        p = PR.softmax64(s, 1) if logits else s.astype(np.float64)
        second = np.argsort(-p, axis=1, kind="stable")[:, 1]
        p2 = -np.sort(-p, axis=1)[:, 1]
        # every branch of the rule occurs
        assert (t1 == 15).any() and (t1 == 0).any() and mask.any()
        assert ((second == 15) & (p2 > 0.3)).any() and ((second == 15) & (p2 < 0.3)).any()
        b = PR.make_boundary_scores(2, 16, 16, 6, 0.7, logits=logits)
        mb, _ = PR.seeds(s, 15, 0.7, from_logits=logits, boundary_scores=b)
        assert mb.any() and not mb.all()


def test_signatures_hold_the_parcel_entry_points():
    from crop2seg_amd import _lib
    for name in ("c2s_parcel_seeds", "c2s_label_components_workspace_bytes", "c2s_label_components",
                 "c2s_parcel_vote_workspace_bytes", "c2s_parcel_vote"):
        assert name in _lib.SIGNATURES, name


def test_argument_validation_without_gpu():
    """Bad arguments return C2S_EINVAL (-1) with a message before any launch."""
    from crop2seg_amd import _lib
    L = _lib.lib()
    p = 4096                                                   # a non-NULL, 16-byte aligned stand-in: never dereferenced

    def refused(rc, word):
        return rc == -1 and word in L.c2s_last_error()

    assert refused(L.c2s_parcel_seeds(None, None, p, None, 1, 16, 8, 8, 1, 15, 0.3, None), b"null")
    assert refused(L.c2s_parcel_seeds(p, None, None, None, 1, 16, 8, 8, 1, 15, 0.3, None), b"null")
    assert refused(L.c2s_parcel_seeds(p, None, p, None, 1, 1, 8, 8, 1, 15, 0.3, None), b"K <= 32")
    assert refused(L.c2s_parcel_seeds(p, None, p, None, 1, 33, 8, 8, 1, 15, 0.3, None), b"K <= 32")
    assert refused(L.c2s_parcel_seeds(p, None, p, None, 1, 16, 8, 8, 2, 15, 0.3, None), b"from_logits")
    assert refused(L.c2s_parcel_seeds(p, None, p, None, 0, 16, 8, 8, 1, 15, 0.3, None), b"shape")

    need = L.c2s_label_components_workspace_bytes(3, 37, 53)
    assert need == (2 * 3 * 37 * 53 + 3 * -(-37 * 53 // 256)) * 4
    assert L.c2s_label_components_workspace_bytes(0, 8, 8) == 0 and L.c2s_label_components_workspace_bytes(2, 1 << 15, 1 << 15) == 0
    assert refused(L.c2s_label_components(None, p, p, 3, 37, 53, 13, p, need, p, None), b"null")
    assert refused(L.c2s_label_components(p, p, p, 3, 37, 53, 13, None, need, p, None), b"null")
    assert refused(L.c2s_label_components(p, p, p, 3, 37, 53, 13, p, need, None, None), b"null")
    assert refused(L.c2s_label_components(p, p, p, 3, 37, 53, 0, p, need, p, None), b"min_size")
    assert refused(L.c2s_label_components(p, p, p, 3, 37, 53, 13, p, need - 1, p, None), b"needed")
    assert refused(L.c2s_label_components(p, p, p, 3, 37, 53, 13, p + 4, need, p, None), b"aligned")
    assert refused(L.c2s_label_components(p, p, p, 3, 0, 53, 13, p, need, p, None), b"shape")

    need = L.c2s_parcel_vote_workspace_bytes(2, 7, 16)
    assert need == 2 * 7 * 16 * 4 and L.c2s_parcel_vote_workspace_bytes(2, 0, 16) == 0
    ok = dict(B=2, H=8, W=8, K=16, cap=7, bg=0.75, outside=0, ws=p, n=need, err=p)

    def vote(pred=p, labels=p, out=p, pc=p, **kw):
        a = dict(ok, **kw)
        return L.c2s_parcel_vote(pred, labels, out, pc, a["B"], a["H"], a["W"], a["K"], a["cap"], a["bg"], a["outside"], a["ws"],
                                 a["n"], a["err"], None)

    assert refused(vote(pred=None), b"null") and refused(vote(labels=None), b"null") and refused(vote(out=None), b"null")
    assert refused(vote(pc=None), b"null") and refused(vote(ws=None), b"null") and refused(vote(err=None), b"null")
    assert refused(vote(K=1), b"K <= 32") and refused(vote(K=33), b"K <= 32")
    assert refused(vote(cap=0), b"cap")
    assert refused(vote(outside=2), b"outside")
    assert refused(vote(bg=float("nan")), b"NaN")
    assert refused(vote(n=need - 1), b"needed")
    assert refused(vote(ws=p + 8), b"aligned")
    assert refused(vote(W=0), b"shape")


def test_python_entry_points_refuse_cpu_tensors():
    import torch
    from crop2seg_amd import postprocess as PP
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.parcel_seeds(torch.zeros(1, 16, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.label_components(torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.homogenize(torch.zeros(1, 8, 8, dtype=torch.int64), torch.zeros(1, 8, 8, dtype=torch.int32), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PP.homogenize_boundaries(torch.zeros(1, 16, 8, 8))
