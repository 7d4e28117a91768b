"""tests/tail_ref.py checked on the CPU: its float64 formulas agree with torch and oracle/tail_oracle.py at 1e-12, the per-element
bound is calibrated against the references alone (a float32 evaluation of the same formulas stays <= 1 on every row of the
tables of tests/test_tail_reference_gpu.py and meets the existing scalar and Frobenius bars), and planted faults of the
kind the existing bars let through reach ratio >= 10 (integer outputs: a mismatch)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R
import test_tail_reference_gpu as T
from oracle import tail_oracle as TO

TIGHT = 1e-12


def close(a, b, tol=TIGHT):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def small(rows, limit=1000):
    return [r for r in rows if r["B"] * r["H"] * r["W"] <= limit]


# ------------------------------------------------------------------------------------------------ the references vs torch
@pytest.mark.parametrize("row", [r for r in small(T.CE_ROWS) if not r.get("bad")], ids=lambda r: r["name"])
def test_ce_ref_is_torch_cross_entropy(row):
    z, t, kw = T.ce_args(row)
    ref, _ = T.reference("ce", row)
    zz = z.double().requires_grad_(True)
    w = None if kw["class_w"] is None else kw["class_w"].double()
    loss = F.cross_entropy(zz, t, weight=w, ignore_index=kw["ignore_index"],
                           label_smoothing=float(np.float32(kw["label_smoothing"])))
    loss.backward()
    assert close(ref["loss"], loss.detach().reshape(1)) and close(ref["glogits"], zz.grad)


def test_ce_ref_all_ignored_is_nan_like_torch():
    z, t, kw = T.ce_args(T.CE_ALL_IGNORED)
    ref, _ = R.ce_ref(z, t, **kw)
    assert bool(torch.isnan(ref["loss"]).all()) and bool((ref["glogits"] == 0).all())
    assert bool(torch.isnan(F.cross_entropy(z.double(), t, label_smoothing=0.1)))


def focal_written_out(z, t, gamma, ignore_index, w, size_average):
    K = z.shape[1]
    zr = z.permute(0, 2, 3, 1).reshape(-1, K)
    tf = t.reshape(-1)
    keep = (tf != ignore_index) & (tf >= 0) & (tf < K)
    lpt = F.log_softmax(zr[keep], 1).gather(1, tf[keep][:, None])[:, 0]
    f = -(1 - lpt.exp()) ** gamma * lpt
    if w is None:
        return f.mean() if size_average else f.sum()
    wt = w[tf[keep]]
    return wt.mean() * f.mean() if size_average else wt.sum() * f.sum()


@pytest.mark.parametrize("row", [r for r in small(T.FOCAL_ROWS) if r["K"] > 1 or r["gamma"] >= 1], ids=lambda r: r["name"])
def test_focal_ref_is_autograd_of_the_written_out_loss(row):
    z, t, kw = T.focal_args(row)
    ref, _ = T.reference("focal", row)
    zz = z.double().requires_grad_(True)
    w = None if kw["class_w"] is None else kw["class_w"].double()
    g32 = float(np.float32(kw["gamma"]))
    loss = focal_written_out(zz, t, g32, kw["ignore_index"], w, kw["size_average"])
    loss.backward()
    prior = 0.0 if kw["prior"] is None else float(kw["prior"])
    assert close(ref["loss"], loss.detach().reshape(1) + prior)
    assert close(ref["glogits"], zz.grad)
    if not row.get("bad"):
        orc = TO.focal_ce(z.double(), t, g32, kw["ignore_index"], w, kw["size_average"])
        assert close(ref["loss"], orc.reshape(1) + prior)


@pytest.mark.parametrize("row", [r for r in small(T.SMOOTH_ROWS, 5000) if not r.get("bad")], ids=lambda r: r["name"])
def test_smooth_ref_is_autograd_of_the_written_out_loss(row):
    z, t, kw = T.smooth_args(row)
    ref, _ = T.reference("smooth", row)
    K = z.shape[1]
    ls = float(np.float32(kw["label_smoothing"]))
    dil = TO.get_dilated(t, K, 4).double()                       # the oracle's smooth_targets, in float64
    nd = dil.sum(1, keepdim=True)
    targets = torch.where(dil == 1, (1 - ls / K * (K - nd)) / nd, torch.full_like(dil, ls / K))
    # the oracle's smooth_targets returns float32, so 1e-6 is all it can give; the ties at 1e-12 are the class masks (bit for
    # bit against get_dilated, test_class_masks_are_the_dilated_one_hot) and CrossEntropyLoss on these float64 targets below
    assert close(targets, TO.smooth_targets(t, K, ls), 1e-6)
    if kw["bg"] is not None:
        targets = torch.where(t[:, None] == kw["bg_index"], kw["bg"].double()[None, :, None, None], targets)
    zz = z.double().requires_grad_(True)
    w = None if kw["class_w"] is None else kw["class_w"].double()
    crit = torch.nn.CrossEntropyLoss(weight=w, reduction=kw["reduction"])(zz, targets)
    value = crit if kw["reduction"] != "none" else crit.sum()
    value.backward()
    assert close(ref["loss"], value.detach().reshape(1)) and close(ref["glogits"], zz.grad)
    if kw["reduction"] == "none":
        assert close(ref["pixel_loss"], crit.detach())
    ww = torch.ones(K, dtype=torch.float64) if w is None else w
    pl = -(ww[None, :, None, None] * targets * F.log_softmax(z.double(), 1)).sum(1)
    assert close(ref["pixel_loss"], pl)


def test_class_masks_are_the_dilated_one_hot():
    for row in small(T.SMOOTH_ROWS, 5000):
        if row.get("bad"):
            continue
        _, t, _ = T.smooth_args(row)
        mask, ok = R.class_masks(t, row["K"])
        assert bool(ok.all()) and bool((mask.permute(0, 3, 1, 2) == TO.get_dilated(t, row["K"], 4).bool()).all())


def test_adam_ref_is_torch_optim_adam():
    gen = torch.Generator().manual_seed(7)
    hp = dict(lr=float(np.float32(1e-3)), betas=(float(np.float32(0.9)), float(np.float32(0.999))), eps=float(np.float32(1e-8)))
    p = torch.nn.Parameter(torch.randn(300, generator=gen).double())
    opt = torch.optim.Adam([p], **hp)
    mine, m, v = p.detach().clone(), torch.zeros(300, dtype=torch.float64), torch.zeros(300, dtype=torch.float64)
    for step in range(1, 6):
        g = torch.randn(300, generator=gen)
        p.grad = g.double() * float(np.float32(0.125))
        opt.step()
        o, _ = R.adam_ref(mine, g, m, v, step, grad_scale=0.125, bounds=False)
        assert close(o["upd"], o["p"] - mine)
        mine, m, v = o["p"], o["m"], o["v"]
        assert close(mine, p.detach()) and close(m, opt.state[p]["exp_avg"]) and close(v, opt.state[p]["exp_avg_sq"])


@pytest.mark.parametrize("row", [r for r in T.METRIC_ROWS if r["name"] != "metrics_grid"], ids=lambda r: r["name"])
def test_metrics_ref_is_argmax_and_topk(row):
    K = row["K"]
    for call in range(2):
        z, t = T.make_metric_inputs(row, call)
        pred, top2, conf, conf2 = R.metrics_ref(z, t)
        finite = torch.isfinite(z).all(1)
        assert bool((torch.from_numpy(pred)[finite] == z.argmax(1)[finite]).all())
        nan_first = torch.isnan(z).float().argmax(1)
        has_nan = torch.isnan(z).any(1)
        assert bool((torch.from_numpy(pred)[has_nan] == nan_first[has_nan]).all()), "NaN counts as the maximum"
        i1, i2 = R.metrics_scan(z)
        assert np.array_equal(i1, pred.reshape(-1)), "the scan form and the argmax form disagree"
        assert np.array_equal(np.where(t.reshape(-1).numpy() == i2, i2, i1), top2.reshape(-1))
        if K >= 3:
            distinct = TO.top2_defined(z) & finite
            tk = z.topk(2, dim=1).indices
            assert bool(distinct.any())
            assert bool((torch.from_numpy(i2).reshape(t.shape)[distinct] == tk[:, 1][distinct]).all())
        ok = (t >= 0) & (t < K) & finite
        if K < 2:
            continue
        zz, tt = z.permute(0, 2, 3, 1)[ok].t()[None, :, :, None], t[ok][None, :, None]
        o_pred, o_top2, o_conf, o_conf2 = TO.metrics_tail(zz, tt, K)
        p2, t2, c1, c2 = R.metrics_ref(zz, tt)
        assert np.array_equal(c1, o_conf) and np.array_equal(c2, o_conf2) and np.array_equal(p2, o_pred.numpy())


@pytest.mark.parametrize("row", T.BOUNDARY_ROWS[:3], ids=lambda r: r["name"])
def test_label_refs_are_the_oracle(row):
    y = T.make_labels(row)
    assert np.array_equal(R.boundary_target_ref(y), TO.boundary_target(y, 4).numpy())
    assert np.array_equal(R.region_relabel_ref(y, 1, 3), TO.region_target(y, 4, "boundary", -1).numpy())
    assert np.array_equal(R.region_relabel_ref(y, 0, 3), TO.region_target(y, 4, "interior", -1).numpy())
    b = R.boundary_target_ref(y)
    assert 0 < b.sum() < b.size or b.size <= 10


def test_confusion_add_ref_is_bincount():
    gen = torch.Generator().manual_seed(3)
    p, t = torch.randint(0, 15, (500,), generator=gen), torch.randint(0, 15, (500,), generator=gen)
    assert np.array_equal(R.confusion_add_ref(p, t, 15), TO.confusion_matrix(p.numpy(), t.numpy(), 15))
    p[::5], t[1::7] = 15, -1
    ok = (p < 15) & (t >= 0)
    assert np.array_equal(R.confusion_add_ref(p, t, 15), TO.confusion_matrix(p[ok].numpy(), t[ok].numpy(), 15))


# ------------------------------------------------------------------------------------------------ the tables themselves
def test_tables_reach_every_path():
    T.assert_table_coverage()


def test_saturated_rows_saturate_in_float32():
    for row in T.FOCAL_ROWS + T.CE_ROWS:
        if row.get("logits") != "sat":
            continue
        z, t, _ = R.make_loss_inputs(row)
        sat = R.saturated(z, t)
        valid = (t.reshape(-1) >= 0) & (t.reshape(-1) < row["K"])
        assert bool(sat[::2][valid[::2]].all()), f"{row['name']}: a pixel built to saturate has pt != 1.f"
        if row["K"] > 1:
            assert int(sat.sum()) >= 1 and not bool(sat[1::2].all())


def test_references_and_bounds_are_finite():
    for kind, rows in (("ce", T.CE_ROWS), ("focal", T.FOCAL_ROWS), ("smooth", T.SMOOTH_ROWS)):
        for row in rows:
            ref, A = T.reference(kind, row)
            for k in ref:
                assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(A[k]).all()), (row["name"], k)


# ------------------------------------------------------------------------------------------------ calibration: float32
def calibrate(row, ref, A, out32, bars):
    worst = {}
    for name in ref:
        assert bool(torch.isfinite(out32[name]).all()), f"{row['name']} {name}: the float32 evaluation is not finite"
        worst[name] = R.bound_ratio(out32[name], ref[name], A[name])
        assert worst[name] <= 1.0, f"{row['name']} {name}: float32 evaluation at ratio {worst[name]:.3f} > 1"
    for name, (kind, bar) in bars.items():
        if name not in ref:
            continue
        err = out32[name].double() - ref[name]
        if kind == "frob":
            assert float(err.norm() / (ref[name].norm() + 1e-30)) <= bar, (row["name"], name)
        else:
            assert float(err.abs().max()) <= bar * float(ref[name].abs().max()), (row["name"], name)
    return worst


LOSS_BARS = {"loss": ("max", R.SCALAR_REL), "glogits": ("max", R.GRAD_MAX_REL)}


@pytest.mark.parametrize("row", T.CE_ROWS, ids=lambda r: r["name"])
def test_fp32_evaluation_ce(row):
    z, t, kw = T.ce_args(row)
    ref, A = T.reference("ce", row)
    calibrate(row, ref, A, R.ce_ref(z, t, dtype=torch.float32, **kw)[0], LOSS_BARS)


@pytest.mark.parametrize("row", T.FOCAL_ROWS, ids=lambda r: r["name"])
def test_fp32_evaluation_focal(row):
    z, t, kw = T.focal_args(row)
    ref, A = T.reference("focal", row)
    calibrate(row, ref, A, R.focal_ref(z, t, dtype=torch.float32, **kw)[0], LOSS_BARS)


@pytest.mark.parametrize("row", T.SMOOTH_ROWS, ids=lambda r: r["name"])
def test_fp32_evaluation_smooth(row):
    z, t, kw = T.smooth_args(row)
    ref, A = T.reference("smooth", row)
    bars = {"loss": ("max", R.SCALAR_REL), "glogits": ("max", 2e-6), "pixel_loss": ("max", 4e-6)}
    calibrate(row, ref, A, R.smooth_ref(z, t, dtype=torch.float32, **kw)[0], bars)


@pytest.mark.parametrize("row", T.ADAM_ROWS, ids=lambda r: r["name"])
def test_fp32_evaluation_adam(row):
    p, g, m, v, off, n = R.make_adam_inputs(row)
    s = slice(off, off + n)
    ref, A = T.reference("adam", row)
    out32, _ = R.adam_ref(p[s], g[s], m[s], v[s], dtype=torch.float32, **T.adam_kwargs(row))
    out32 = dict(out32, upd=out32["p"].double() - p[s].double())       # as the GPU test measures it: from the stored p
    bars = {k: ("frob", R.ADAM_FROB) for k in ("p", "m", "v")}
    bars["upd"] = ("frob", R.adam_upd_frob(ref, A))
    calibrate(row, ref, A, out32, bars)


def test_adam_run_reference_is_usable():
    p64, single = T.adam_run_reference()
    assert bool(torch.isfinite(p64).all()) and 0 < single < R.ADAM_FROB
    print(f"one float32 Adam step of the reference: Frobenius error of p {single:.3e}")


# ------------------------------------------------------------------------------------------------ planted faults
def fault_ratio(kind, rows, fault, outputs):
    """The largest ratio a planted fault reaches over the rows, on the named outputs."""
    fn = {"ce": (T.ce_args, R.ce_ref), "focal": (T.focal_args, R.focal_ref), "smooth": (T.smooth_args, R.smooth_ref)}[kind]
    worst = 0.0
    for row in rows:
        z, t, kw = fn[0](row)
        ref, A = T.reference(kind, row)
        bad, _ = fn[1](z, t, bounds=False, fault=fault, **kw)
        for name in outputs:
            worst = max(worst, R.bound_ratio(bad[name], ref[name], A[name]))
    return worst


def by_name(rows, *names):
    return [r for r in rows if r["name"] in names]


def test_planted_lost_block_partial():
    """The block that only the second grid pass of ce_fwd reaches: ce_grid is the row that holds it (no row of
    tests/test_ops_gpu.py or tests/test_tail_gpu.py has more than 65536 pixels, so none could see this fault)."""
    row, = by_name(T.CE_ROWS, "ce_grid")
    assert row["B"] * row["H"] * row["W"] >= T.CE_CAP + 256
    assert fault_ratio("ce", [row], "partial", ("loss", "tot")) >= 10


def test_planted_wrong_last_class_row():
    assert fault_ratio("ce", [r for r in small(T.CE_ROWS) if r["K"] > 2], "last_class", ("glogits",)) >= 10


def test_planted_smoothing_over_k_minus_1():
    assert fault_ratio("ce", [r for r in small(T.CE_ROWS) if r["K"] > 1 and r.get("ls", 0) > 0], "smooth_k",
                       ("loss", "glogits")) >= 10


def test_planted_neighbour_across_the_batch_boundary():
    assert fault_ratio("smooth", by_name(T.SMOOTH_ROWS, "smooth_batch_edge"), "batch", ("pixel_loss", "glogits", "loss")) >= 10


def test_planted_lost_bit_31():
    rows = by_name(T.SMOOTH_ROWS, "smooth_k32_adjacent", "smooth_k32_adjacent_col")
    assert len(rows) == 2
    for row in rows:
        assert fault_ratio("smooth", [row], "bit31", ("glogits", "loss")) >= 10


def test_planted_focal_coef_without_first_term():
    assert fault_ratio("focal", [r for r in small(T.FOCAL_ROWS) if r["gamma"] > 0 and r["K"] > 1], "no_t1", ("glogits",)) >= 10


@pytest.mark.parametrize("fault", ["bc2_nosqrt", "scale_m_only"])
def test_planted_adam_faults(fault):
    worst = 0.0
    for row in T.ADAM_ROWS:
        if row["n"] > 1000 or (fault == "scale_m_only" and row.get("gs", 1.0) == 1.0):
            continue
        p, g, m, v, off, n = R.make_adam_inputs(row)
        s = slice(off, off + n)
        ref, A = T.reference("adam", row)
        bad, _ = R.adam_ref(p[s], g[s], m[s], v[s], bounds=False, fault=fault, **T.adam_kwargs(row))
        worst = max(worst, R.bound_ratio(bad["upd"], ref["upd"], A["upd"]))
    assert worst >= 10


def test_planted_stale_second_maximum():
    hit = False
    for row in T.METRIC_ROWS[:4]:
        z, t = T.make_metric_inputs(row, 0)
        _, top2, _, conf2 = R.metrics_ref(z, t)
        i1, i2 = R.metrics_scan(z, fault="stale_second")
        tf = t.reshape(-1).numpy()
        hit |= not np.array_equal(np.where(tf == i2, i2, i1), top2.reshape(-1))
    assert hit


def test_planted_transposed_confusion_matrix():
    z, t = T.make_metric_inputs(T.METRIC_ROWS[2], 0)
    _, _, conf, _ = R.metrics_ref(z, t)
    _, _, bad, _ = R.metrics_ref(z, t, fault="transposed")
    assert not np.array_equal(conf, bad) and np.array_equal(conf, bad.T)
