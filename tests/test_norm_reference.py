"""The float64 references of tests/norm_ref.py and their per-element bound, checked on the CPU:

  * independence: every reference agrees to 1e-12 with float64 torch autograd on F.group_norm / F.batch_norm, on the
    squeeze-and-excitation formula and on oracle.temporal_aggregate (which upsamples with F.interpolate);
  * calibration: the same formulas evaluated in float32 (torch's own summation order) stay at |err| <= 1 * u * A on every
    row of the GPU tables (the rows sized by CU count scaled down) -- the constant C_BOUND = 2 of the GPU tests is this plus a
    margin, fitted to no kernel;
  * the kink builders converge on every row with no element left out;
  * the checker's own tests: planted faults give a ratio |err| / (u A) >= 10 on at least one output while the clean fp32
    evaluation of the same inputs passes (several of them pass the Frobenius bars of tests/test_ops_gpu.py).
"""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from norm_ref import U, assert_within, bound_ratio

CUS = 4          # the wrapping rows at the size of a 4-CU device


def close(name, got, ref):
    err = float((got.double() - ref.double()).abs().max())
    assert err <= 1e-12 * (float(ref.double().abs().max()) + 1e-30) + 1e-300, f"{name}: {err:.3e}"


def ratios(o32, o, A, skip=("pre", "z1")):
    return {k: bound_ratio(o32[k], o[k], A[k]) for k in A if k in o32 and k not in skip}


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("kind,training,use_valid,use_res,relu", [
    ("group", True, True, True, True), ("group", True, False, False, False), ("batch", True, True, True, True),
    ("batch", True, False, False, True), ("batch", False, True, True, True), ("batch", False, False, False, False)])
def test_norm_ref_agrees_with_autograd(kind, training, use_valid, use_res, relu):
    g = torch.Generator().manual_seed(1)
    N, C, H, W = 4, 8, 5, 7
    x = (torch.randn(N, C, H, W, generator=g, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gam = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    bet = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True) if use_res else None
    go = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    valid = torch.ones(N, dtype=torch.bool)
    if use_valid:
        valid[1] = False
    rm2, rv2 = rm.clone(), rv.clone()
    xs = x[valid]
    y = F.group_norm(xs, 4, gam, bet, 1e-5) if kind == "group" else F.batch_norm(xs, rm2, rv2, gam, bet, training, 0.1, 1e-5)
    y = F.relu(y) if relu else y
    if use_res:
        y = y + res[valid]
    y.backward(go[valid])
    o, _ = R.norm_ref(x, gam, bet, kind, 4, training, (rm, rv), res, relu, valid, go)
    close("y", o["y"], y.detach())
    close("gx", o["gx"], x.grad[valid])
    close("dgamma", o["dgamma"], gam.grad)
    close("dbeta", o["dbeta"], bet.grad)
    if use_res:
        close("g_residual", o["g_residual"], res.grad[valid])
    if kind == "group" or not training:
        close("dbias", o["dbias"], x.grad[valid].sum((0, 2, 3)))
    if kind == "batch" and training:
        close("running_mean", o["running_mean"], rm2)
        close("running_var", o["running_var"], rv2)
    # group_stats: (mean, rstd) of the group
    xv = xs.detach()
    if kind == "group":
        xg = xv.reshape(xv.shape[0], 4, -1)
        m, v = xg.mean(-1), xg.var(-1, unbiased=False)
    elif training:
        m, v = xv.mean((0, 2, 3)), xv.var((0, 2, 3), unbiased=False)
    else:
        m, v = rm, rv
    close("group mean", o["group_stats"][..., 0], m)
    close("group rstd", o["group_stats"][..., 1], (v + 1e-5).rsqrt())


def test_norm_ref_without_affine_is_instance_norm():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 6, 4, 4, generator=g, dtype=torch.float64, requires_grad=True)
    go = torch.randn(3, 6, 4, 4, generator=g, dtype=torch.float64)
    y = F.instance_norm(x, eps=1e-5)
    y.backward(go)
    o, _ = R.norm_ref(x, None, None, "group", 6, relu=False, gout=go)
    close("y", o["y"], y.detach())
    close("gx", o["gx"], x.grad)


@pytest.mark.parametrize("use_valid,prior", [(True, True), (False, False)])
def test_se_ref_agrees_with_autograd(use_valid, prior):
    g = torch.Generator().manual_seed(3)
    N, C, H, W = 3, 32, 5, 6
    x = torch.randn(N, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    w1 = (torch.randn(C // 16, C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    w2 = (torch.randn(C, C // 16, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    go = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    p1 = torch.randn(C // 16, C, generator=g, dtype=torch.float64) if prior else None
    p2 = torch.randn(C, C // 16, generator=g, dtype=torch.float64) if prior else None
    valid = torch.ones(N, dtype=torch.bool)
    if use_valid:
        valid[0] = False
    xs = x[valid]
    s = torch.sigmoid(F.linear(F.relu(F.linear(xs.mean(dim=(2, 3)), w1)), w2))
    y = xs * s[:, :, None, None]
    y.backward(go[valid])
    o, _ = R.se_ref(x, w1, w2, valid, go, p1, p2)
    assert bool((o["z1"] > 0).any()), "every hidden unit dead: the check is empty"
    close("y", o["y"], y.detach())
    close("gx", o["gx"], x.grad[valid])
    close("gW1", o["gW1"], w1.grad + (p1 if prior else 0))
    close("gW2", o["gW2"], w2.grad + (p2 if prior else 0))


@pytest.mark.parametrize("mode", ["att_group", "att_mean", "mean"])
@pytest.mark.parametrize("shape", [(2, 3, 32, 16, 8, 16, 4, 4), (1, 4, 64, 16, 16, 8, 2, 4), (2, 2, 16, 16, 8, 8, 8, 8)])
def test_agg_ref_agrees_with_the_oracle(mode, shape):
    """oracle.temporal_aggregate takes its taps from F.interpolate; the reference writes them out."""
    from oracle import crop2seg_oracle as O
    B, T, C, nh, H, W, h, w = shape
    if mode == "mean":
        h = w = 1
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T, C, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    attn = torch.softmax(torch.randn(nh, B, T, h, w, generator=g, dtype=torch.float64), dim=2).requires_grad_(True)
    go = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    valid = torch.ones(B, T, dtype=torch.bool)
    valid[0, 1] = False
    ref = O.temporal_aggregate(x, ~valid, attn, mode)
    ref.backward(go)
    o, _ = R.agg_ref(x, None if mode == "mean" else attn, valid, go, mode, n_head=nh)
    close("out", o["out"], ref.detach())
    close("gx", o["gx"], x.grad)
    if mode != "mean":
        close("gattn", o["gattn"], attn.grad)


def test_bilinear_matrix_is_torchs_upsampling():
    for n_in, n_out in ((4, 8), (2, 16), (8, 32), (1, 4), (3, 12), (5, 5)):
        e = torch.eye(n_in, dtype=torch.float64)
        ref = F.interpolate(e[None], size=n_out, mode="linear", align_corners=False)[0].T
        close(f"{n_in}->{n_out}", R.bilinear_matrix(n_in, n_out), ref)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_pixel_gn_ref_agrees_with_autograd(p):
    g = torch.Generator().manual_seed(5)
    B, C, h = 2, 64, 3
    x = torch.randn(B, C, h, h, generator=g, dtype=torch.float64, requires_grad=True)
    gam = (1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    bet = (0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    keep = (torch.rand(B * h * h, C, generator=g) >= p).double()
    go = torch.randn(B, C, h, h, generator=g, dtype=torch.float64)
    xp = x.permute(0, 2, 3, 1).reshape(B * h * h, C)
    ref = F.group_norm(xp * keep / (1 - p), 16, gam, bet, 1e-5).view(B, h, h, C).permute(0, 3, 1, 2)
    ref.backward(go)
    o, _ = R.pixel_gn_ref(x, keep, p, gam, bet, 16, go)
    close("y", o["y"], ref.detach())
    close("gx", o["gx"], x.grad)
    close("dgamma", o["dgamma"], gam.grad)
    close("dbeta", o["dbeta"], bet.grad)


# ------------------------------------------------------------------------------------------------ calibration, kink builders
def _fp32_within_one(o32, o, A):
    r = ratios(o32, o, A)
    assert r and max(r.values()) <= 1.0, {k: round(v, 3) for k, v in r.items()}
    return r


@pytest.mark.parametrize("row", R.norm_rows(CUS), ids=lambda r: r["name"])
def test_fp32_evaluation_of_norm_rows_stays_within_one(row):
    t = R.norm_inputs(row)
    assert t["kink_rounds"] <= 8
    o, A = R.norm_row_ref(row, t)
    if row.get("relu", True):                     # the builder left no element on the kink (none is excluded below)
        assert bool((o["pre"].abs() > R.KINK * U * A["pre"]).all())
    assert all(bool(torch.isfinite(v).all()) for v in list(o.values()) + list(A.values())), "a padded frame leaked"
    o32 = R.norm_row_ref(row, t, dtype=torch.float32)[0]
    _fp32_within_one(o32, o, A)
    for k in ratios(o32, o, A):                   # and the Frobenius bars the GPU file applies, as norm_frob states them
        assert_within(f"{row['name']} {k}", o32[k], o[k], A[k], 1.0, R.norm_frob(row, k))


@pytest.mark.parametrize("row", R.se_rows(), ids=lambda r: r["name"])
def test_fp32_evaluation_of_se_rows_stays_within_one(row):
    t = R.se_inputs(row)
    assert t["kink_rounds"] <= 8
    o, A = R.se_row_ref(row, t)
    assert bool((o["z1"].abs() > R.KINK * U * A["z1"]).all()) and bool((o["z1"] > 0).any())
    assert all(bool(torch.isfinite(v).all()) for v in list(o.values()) + list(A.values())), "a padded frame leaked"
    _fp32_within_one(R.se_row_ref(row, t, dtype=torch.float32)[0], o, A)


@pytest.mark.parametrize("row", R.agg_rows(), ids=lambda r: r["name"])
def test_fp32_evaluation_of_agg_rows_stays_within_one(row):
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    assert all(bool(torch.isfinite(v).all()) for v in list(o.values()) + list(A.values())), "a padded frame leaked"
    _fp32_within_one(R.agg_row_ref(row, t, dtype=torch.float32)[0], o, A)


@pytest.mark.parametrize("row", R.pixel_gn_rows(), ids=lambda r: r["name"])
def test_fp32_evaluation_of_pixel_gn_rows_stays_within_one(row):
    t = R.pixel_gn_inputs(row)
    o, A = R.pixel_gn_row_ref(row, t)
    _fp32_within_one(R.pixel_gn_row_ref(row, t, dtype=torch.float32)[0], o, A)


def test_row_tables_reach_every_instance_and_branch():
    """What the closing test of the GPU file asserts about the kernels reached, from the shapes alone."""
    rows = R.norm_rows(256)
    inst = {(R.onepass_instance(r), bool(r.get("res")), r["kind"]) for r in rows if R.onepass_instance(r)}
    assert inst == {(nk, res, kind) for nk in (1, 2, 4, 8) for res in (False, True) for kind in ("group", "batch")}
    br = set().union(*(R.two_pass_branches(r["H"] * r["W"]) for r in rows))
    assert br == {"full", "full_unaligned", "float4_tail", "scalar"}
    wrap = [r for r in rows if "wrap" in r["name"]]
    for r in wrap:
        quads = r["N"] * r["C"] * (r["H"] * r["W"] // 256) // 4
        assert R.onepass_instance(r) and quads >= 2.5 * 8 * 256
    assert not R.onepass_instance(next(r for r in rows if r["name"] == "g_over_512_waves"))
    assert not R.onepass_instance(next(r for r in rows if r["name"] == "g_wpg3"))
    assert R.onepass_instance(next(r for r in rows if r["name"] == "g_limit_512_waves")) == 8


# ------------------------------------------------------------------------------------------------ the checker's own tests
def _row(rows, name):
    return next(r for r in rows if r["name"] == name)


def _clean_and_faulty(o, A, clean, faulty, frob):
    """The clean fp32 evaluation passes the full check; the faulty one has a ratio >= 10 on at least one output."""
    for k in ratios(clean, o, A):
        assert_within(k, clean[k], o[k], A[k], R.C_BOUND, frob(k))
    r = ratios(faulty, o, A)
    assert max(r.values()) >= 10.0, {k: round(v, 3) for k, v in r.items()}
    return r


@pytest.mark.parametrize("name", ["g_nk2_off30", "g_nk8_off1000", "g_80_off30", "b_nk2_off30"])
def test_planted_one_pass_variance_is_caught(name):
    row = _row(R.norm_rows(CUS), name)
    t = R.norm_inputs(row)
    o, A = R.norm_row_ref(row, t)
    clean, _ = R.norm_row_ref(row, t, dtype=torch.float32)
    bad, _ = R.norm_row_ref(row, t, dtype=torch.float32, variance="naive")
    r = _clean_and_faulty(o, A, clean, bad, lambda k: R.norm_frob(row, k))
    assert r["y"] >= 10.0 and r["gx"] >= 10.0


def test_planted_single_element_passes_frobenius_and_is_caught():
    """One element of 2,097,152 scaled by 1 + 1e-4: far inside the 2e-6 Frobenius bar, far outside the bound."""
    row = dict(name="gn_2m", kind="group", N=2, C=64, H=128, W=128, groups=4)
    t = R.norm_inputs(row)
    o, A = R.norm_ref(t["x"], t["gamma"], t["beta"], "group", 4, relu=True)
    clean, _ = R.norm_ref(t["x"], t["gamma"], t["beta"], "group", 4, relu=True, dtype=torch.float32)
    assert_within("y", clean["y"], o["y"], A["y"], R.C_BOUND, R.FROB["y"])
    bad = clean["y"].clone()
    i = int(torch.argmax(bad.flatten()))
    bad.view(-1)[i] *= 1 + 1e-4
    fr = float((bad.double() - o["y"]).norm() / o["y"].norm())
    assert fr < R.FROB["y"], fr
    assert bound_ratio(bad, o["y"], A["y"]) >= 10.0
    with pytest.raises(AssertionError, match="beyond c \\* u \\* A"):
        assert_within("y", bad, o["y"], A["y"], R.C_BOUND, R.FROB["y"])


def test_planted_neighbour_gamma_is_caught():
    row = _row(R.norm_rows(CUS), "g_nk4_norelu")
    t = R.norm_inputs(row)
    o, A = R.norm_row_ref(row, t)
    clean, _ = R.norm_row_ref(row, t, dtype=torch.float32)
    gam = t["gamma"].clone()
    gam[5] = t["gamma"][6]                         # one channel row takes its neighbour's gain
    bad, _ = R.norm_row_ref(row, dict(t, gamma=gam), dtype=torch.float32)
    r = _clean_and_faulty(o, A, clean, bad, lambda k: R.norm_frob(row, k))
    assert r["y"] >= 10.0


def test_planted_lost_last_segment_is_caught():
    """Statistics from the full 2048-float segment only (HW = 2304: the ragged 256-float segment left out)."""
    row = _row(R.norm_rows(CUS), "g_48_ragged")
    t = R.norm_inputs(row)
    o, A = R.norm_row_ref(row, t)
    clean, _ = R.norm_row_ref(row, t, dtype=torch.float32)
    xs = t["x"][t["valid"]]
    n, C = xs.shape[:2]
    x4 = xs.reshape(n, 4, C // 4, -1)
    m = x4[..., :2048].mean((2, 3), keepdim=True)
    var = ((x4[..., :2048] - m) ** 2).mean((2, 3), keepdim=True)
    y = ((x4 - m) / torch.sqrt(var + 1e-5)).reshape(xs.shape) * t["gamma"].view(1, C, 1, 1) + t["beta"].view(1, C, 1, 1)
    bad = dict(clean, y=y.clamp_min(0))
    r = _clean_and_faulty(o, A, clean, bad, lambda k: R.norm_frob(row, k))
    assert r["y"] >= 10.0


def test_planted_padded_frame_in_batch_statistics_is_caught():
    row = _row(R.norm_rows(CUS), "b_flags")
    t = R.norm_inputs(row)
    o, A = R.norm_row_ref(row, t)
    clean, _ = R.norm_row_ref(row, t, dtype=torch.float32)
    g = torch.Generator().manual_seed(9)
    full = {k: torch.where(torch.isnan(t[k]), torch.randn(t[k].shape, generator=g), t[k]) for k in ("x", "res", "gout")}
    allv = R.norm_ref(full["x"], t["gamma"], t["beta"], "batch", 4, True, (t["rm"], t["rv"]), full["res"], True, None,
                      full["gout"], dtype=torch.float32)[0]
    v = t["valid"]
    bad = {k: (allv[k][v] if allv[k].dim() == 4 else allv[k]) for k in allv}
    r = _clean_and_faulty(o, A, clean, bad, lambda k: R.norm_frob(row, k))
    assert r["y"] >= 10.0 and r["running_mean"] >= 10.0


def test_planted_align_corners_taps_are_caught():
    row = _row(R.agg_rows(), "cpg2_ratio4_nonsquare")
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    clean, _ = R.agg_row_ref(row, t, dtype=torch.float32)
    bad, _ = R.agg_row_ref(row, t, dtype=torch.float32, align_corners=True)
    frob = {"out": R.FROB["out"], "gx": R.FROB["agg_gx"], "gattn": R.FROB["gattn"]}
    r = _clean_and_faulty(o, A, clean, bad, frob.get)
    assert min(r.values()) >= 10.0


def test_planted_channel_group_mixup_is_caught():
    row = _row(R.agg_rows(), "cpg4_ratio2x8")
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    clean, _ = R.agg_row_ref(row, t, dtype=torch.float32)
    bad, _ = R.agg_row_ref(row, t, dtype=torch.float32, cpg=2)          # g * CPG with the wrong CPG
    frob = {"out": R.FROB["out"], "gx": R.FROB["agg_gx"], "gattn": R.FROB["gattn"]}
    r = _clean_and_faulty(o, A, clean, bad, frob.get)
    assert r["out"] >= 10.0 and r["gx"] >= 10.0


def test_planted_overwritten_gattn_is_caught():
    row = _row(R.agg_rows(), "cpg16_ratio8")
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    clean, _ = R.agg_row_ref(row, t, dtype=torch.float32)
    bad, _ = R.agg_row_ref(row, dict(t, prior_gattn=None), dtype=torch.float32)
    frob = {"out": R.FROB["out"], "gx": R.FROB["agg_gx"], "gattn": R.FROB["gattn"]}
    r = _clean_and_faulty(o, A, clean, bad, frob.get)
    assert r["gattn"] >= 10.0 and r["out"] <= 1.0
