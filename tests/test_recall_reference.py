"""tests/recall_ref.py checked on the CPU: its float64 formulas reproduce the fixtures written from the imported reference
criterion (tests/golden/tail_recall_*.npz, tools/make_golden_recall.py) and a torch restatement at 1e-12, the per-element bound
is calibrated against the reference alone (a float32 evaluation of the same formulas stays <= 1 on every row of the table of
tests/test_recall_reference_gpu.py and meets the scalar and max-relative bars), every planted fault is caught on at least one
row (ratio >= 10; integer outputs: a mismatch), and the C entry point refuses bad arguments before it touches a device."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recall_ref as RR
import tail_ref as R
import test_recall_reference_gpu as T

TIGHT = 1e-12
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_recall_*.npz")))


def close(a, b, tol=TIGHT):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def small(rows, limit=1000):
    return [r for r in rows if T.pixels(r) <= limit]


# ------------------------------------------------------------------------------------------------ (a) the imported reference
def load(path):
    f = np.load(path, allow_pickle=False)
    return torch.from_numpy(f["logits"]), torch.from_numpy(f["target"]), int(f["ignore_index"]), float(f["loss"]), \
        torch.from_numpy(f["glogits"])


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-4])
def test_ref_is_the_imported_criterion(path):
    z, t, ign, loss, g = load(path)
    assert z.dtype == torch.float64 and 200 <= t.numel() <= 400
    ref, _ = RR.recall_ref(z, t, ign)
    assert abs(float(ref["loss"]) - loss) <= R.SCALAR_REL * abs(loss)
    assert float((ref["glogits"] - g).abs().max()) <= R.GRAD_MAX_REL * float(g.abs().max())


def test_fixtures_cover_the_cases():
    """No ignored pixels; ignore_index = -1 with class 1 misclassified; K in {2, 15, 20}; logit ties."""
    assert len(GOLDEN) >= 5
    seen = {"plain": False, "ignored": False, "ties": False, "K": set()}
    for path in GOLDEN:
        z, t, ign, _, _ = load(path)
        K = z.shape[1]
        seen["K"].add(K)
        _, _, gt, fn, bad, _ = RR.recall_counts(z, t, ign)
        assert bad == 0 and (gt > 0).sum() >= 2 and (fn > 0).sum() >= 2          # deviation 1: the reference runs
        if bool((t == ign).any()):
            assert ign == -1 and fn[1] >= 1                                      # deviations 2 and 3
            seen["ignored"] = True
        else:
            seen["plain"] = True
        rows = z.permute(0, 2, 3, 1).reshape(-1, K)
        seen["ties"] |= bool(((rows == rows.max(1, keepdim=True).values).sum(1) > 1).any())
    assert seen["plain"] and seen["ignored"] and seen["ties"] and {2, 15, 20} <= seen["K"]


# ------------------------------------------------------------------------------------------------ (b) a torch restatement
@pytest.mark.parametrize("row", small(T.ROWS), ids=lambda r: r["name"])
def test_ref_is_weighted_torch_cross_entropy(row):
    z, t = T.make_inputs(row)
    ign = T.ignore_index(row)
    ref, _ = T.reference(row)
    K, N = z.shape[1], t.numel()
    valid = (t >= 0) & (t < K) & (t != ign)
    tt = torch.where(valid, t, torch.full_like(t, -100))
    pred = z.argmax(1)
    gt = torch.bincount(t[valid], minlength=K)
    fn = torch.bincount(t[valid & (pred != t)], minlength=K)
    w = (fn.clamp_min(1).double() / gt.clamp_min(1).double()).float()
    assert np.array_equal(w.numpy().view(np.int32), ref["weights"].view(np.int32))
    assert np.array_equal(torch.stack([gt, fn]).numpy(), ref["counts"])
    assert int(((t != ign) & ((t < 0) | (t >= K))).sum()) == ref["bad"]
    zz = z.double().requires_grad_(True)
    ce = F.cross_entropy(zz, tt, reduction="none", ignore_index=-100)
    loss = (w.double()[tt.clamp(0, K - 1)] * ce).sum() / N
    loss.backward()
    assert close(ref["loss"], loss.detach().reshape(1)) and close(ref["glogits"], zz.grad)
    assert close(ref["nll"], ce.detach().reshape(-1))


def test_named_rows_are_what_their_names_say():
    def counts(name):
        row = T.by_name(name)
        z, t = T.make_inputs(row)
        return row, t, RR.recall_counts(z, t, T.ignore_index(row))

    row, t, (_, valid, gt, fn, _, w) = counts("perfect")
    assert valid.all() and fn.sum() == 0 and np.array_equal(w, (1.0 / np.maximum(gt, 1)).astype(np.float32))
    row, t, (_, valid, gt, fn, _, w) = counts("all_wrong")
    assert 0 < valid.sum() < valid.size and np.array_equal(fn, gt) and bool((w[gt > 0] == 1).all())
    row, t, (_, valid, gt, fn, _, _) = counts("one_class")
    assert (gt > 0).sum() == 1 and gt[3] == valid.size
    row, t, (_, valid, gt, fn, bad, w) = counts("all_ignored")
    assert valid.sum() == 0 and bad == 0 and gt.sum() == 0 and bool((w == 1).all())
    ref, A = T.reference(row)
    assert float(ref["loss"]) == 0.0 and bool((ref["glogits"] == 0).all())
    row, t, (_, valid, gt, fn, _, w) = counts("class1_perfect_with_ignored")          # deviation 3
    assert bool((t == row["ignore"]).any()) and gt[1] > 0 and fn[1] == 0 and (fn > 0).sum() >= 2
    assert w[1] == np.float32(1.0 / gt[1])


# ------------------------------------------------------------------------------------------------ the table itself
def test_table_reaches_every_path():
    T.assert_table_coverage()
    assert RR.GRID_PIXELS == T.RECALL_COUNT_CAP == T.RECALL_LOSS_CAP == T.RECALL_BWD_CAP
    assert T.pixels(T.by_name("recall_grid")) >= RR.GRID_PIXELS + 256


def test_references_and_bounds_are_finite():
    for row in T.ROWS:
        ref, A = T.reference(row)
        for k in A:
            assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(A[k]).all()), (row["name"], k)


# ------------------------------------------------------------------------------------------------ (c) calibration: float32
@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r["name"])
def test_fp32_evaluation(row):
    z, t = T.make_inputs(row)
    ref, A = T.reference(row)
    out32, _ = RR.recall_ref(z, t, T.ignore_index(row), dtype=torch.float32)
    for name in A:
        assert bool(torch.isfinite(out32[name]).all()), f"{row['name']} {name}: the float32 evaluation is not finite"
        ratio = R.bound_ratio(out32[name], ref[name], A[name])
        assert ratio <= 1.0, f"{row['name']} {name}: float32 evaluation at ratio {ratio:.3f} > 1"
    for name, bar in (("loss", R.SCALAR_REL), ("glogits", R.GRAD_MAX_REL)):
        err = (out32[name].double() - ref[name]).abs().max()
        assert float(err) <= bar * float(ref[name].abs().max()), (row["name"], name)
    assert np.array_equal(out32["counts"], ref["counts"]) and np.array_equal(out32["weights"], ref["weights"])


# ------------------------------------------------------------------------------------------------ (d) planted faults
def caught(rows, fault):
    """(largest ratio the fault reaches on loss / glogits, an integer output differs) over the rows."""
    worst, differs = 0.0, False
    for row in rows:
        z, t = T.make_inputs(row)
        ref, A = T.reference(row)
        bad, _ = RR.recall_ref(z, t, T.ignore_index(row), bounds=False, fault=fault)
        for name in ("loss", "glogits"):
            worst = max(worst, R.bound_ratio(bad[name], ref[name], A[name]))
        differs |= not (np.array_equal(bad["counts"], ref["counts"])
                        and np.array_equal(bad["weights"].view(np.int32), ref["weights"].view(np.int32)))
    return worst, differs


def test_planted_fn_counts_every_pixel():
    ratio, differs = caught(small(T.ROWS), "fn_all")
    assert differs and ratio >= 10


def test_planted_no_floor_at_perfect_recall():
    ratio, differs = caught([T.by_name("perfect")], "no_floor")
    assert differs and ratio >= 10
    ratio, differs = caught([T.by_name("class1_perfect_with_ignored")], "no_floor")
    assert differs and ratio >= 10


def test_planted_mean_over_valid_pixels():
    rows = [r for r in small(T.ROWS) if r["ignore"] is not None and not r.get("all_ignored") and r["K"] > 1]
    ratio, differs = caught(rows, "mean_valid")
    assert not differs and ratio >= 10


def test_planted_last_maximum_on_ties():
    rows = [r for r in small(T.ROWS) if r.get("logits") == "ties" and r["K"] > 1]
    assert rows
    ratio, differs = caught(rows, "argmax_last")
    assert differs
    ratio, differs = caught([r for r in small(T.ROWS) if r.get("logits", "normal") == "normal"], "argmax_last")
    assert not differs and ratio == 0.0, "without ties the first and the last maximum are the same"


def test_planted_lost_second_grid_pass():
    ratio, differs = caught([T.by_name("recall_grid")], "partial")
    assert not differs and ratio >= 10


# ------------------------------------------------------------------------------------------------ (e) the C entry point
def test_argument_validation_without_gpu():
    """K outside [1, 32], NULL required pointers and a short workspace are refused before any launch."""
    from crop2seg_amd import _lib
    L = _lib.lib()
    need = L.c2s_recall_ce_workspace_floats(3, 257)
    assert need == 3 * 257 + 512 + (2 * 65 + 1) + 32 + 2
    assert L.c2s_recall_ce_workspace_floats(1, 1) < need

    def call(logits=16, target=16, loss=16, K=15, ws=16, ws_floats=need, B=3, HW=257):
        return L.c2s_recall_ce(logits, target, loss, None, None, None, B, K, HW, 255, 0, ws, ws_floats, None)

    for kw, word in ((dict(K=0), b"32"), (dict(K=33), b"32"), (dict(K=-1), b"32"), (dict(logits=None), b"null"),
                     (dict(target=None), b"null"), (dict(loss=None), b"null"), (dict(ws=None), b"null"),
                     (dict(ws_floats=need - 1), b"workspace"), (dict(ws_floats=0), b"workspace"), (dict(B=0), b"bad args"),
                     (dict(HW=0), b"bad args")):
        rc = call(**kw)
        assert rc != 0 and word in L.c2s_last_error() and b"recall_ce" in L.c2s_last_error(), (kw, L.c2s_last_error())


def test_class_refuses_what_the_kernels_cannot_take():
    from crop2seg_amd.learning import losses
    with pytest.raises(ValueError, match="32"):
        losses.RecallCrossEntropy(n_classes=33)
    crit = losses.RecallCrossEntropy()
    assert (crit.n_classes, crit.ignore_index) == (19, 255) and crit.grad() is None and crit.bad_target_count() == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(torch.zeros(1, 19, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="classes"):
        crit(torch.zeros(1, 15, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64))


def test_trainstep_takes_a_criterion_argument():
    import inspect

    from crop2seg_amd.learning.utils import TrainStep
    assert inspect.signature(TrainStep.__init__).parameters["criterion"].default is None
