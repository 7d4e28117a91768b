"""The normalisation, squeeze-and-excitation, temporal-aggregation and dropout + per-pixel GroupNorm kernels against the
float64 references of tests/norm_ref.py, element by element.

tests/test_ops_gpu.py holds these kernels to one Frobenius ratio per tensor against fp32 torch, on 16 shapes whose planes
are all powers of two; a single wrong element of a 2M-element plane passes that bar (test_norm_reference.py plants one).
Here every row of the tables in norm_ref.py goes through the engine entry point a model uses (engine.norm_act,
squeeze_excite, temporal_aggregate, dropout_nchw + pixel_group_norm: tape, workspaces and Workspace.sync_area included) and
checks every output over the real frames against |got - ref| <= 2 u A (u = 2^-24, A = first-order rounding propagation) next
to the Frobenius bars of test_ops_gpu.py.  The padded frames of every input hold NaN: every output must be finite, y of a
padded frame equal to pad_value and its gradient 0 (or bit-identical to the gradient that was there when the kernel
accumulates), group_stats / row_ab of a padded GroupNorm frame 0; row_ab of a real frame is checked by value too.

Normalisation rows run in the two-pass form with the parameter-gradient launch on the side stream and on the main stream,
and in the one-pass form where the shape takes it (a shape it does not take is run once more with the one-pass switch on
and must fall back to the same bits); each row asserts which form c2s_norm_onepass_sync_bytes gives it, the
runs of a row must agree bit for bit (include/c2s_hip.h: "same arithmetic in the same order"), every run shares ONE
workspace (one sync area for launches of every shape, as in a model), and test_reached_instances_and_branches asserts that
the rows reached every (NK, residual, kind) instance of the one-pass kernels and every branch of the two-pass kernels
(scalar / float4 tail / full segment, the latter also at row bases that are not 16-byte aligned).

The constant 2 is not fitted to the kernels (norm_ref.py: a float32 evaluation of the reference formulas stays <= 1 on every
row).  Worst ratios |err| / (u A) observed on an MI355X (printed with -s; for information, the constant does not move):

    family                  y      gx     dgamma  dbeta  dbias  group_stats  row_ab  running_mean  running_var
    two-pass GroupNorm      0.61   0.83   0.22    0.37   0.24   0.61         0.53
    one-pass GroupNorm      0.61   0.83   0.047   0.11   0.055  0.38         0.46
    two-pass BatchNorm      0.70   0.72   0.17    0.25   0.37   0.61         0.53    0.87          0.58
    one-pass BatchNorm      0.70   0.72   0.16    0.23   0.054  0.52         0.53    0.87          0.58
    dropout + pixel GN      0.42   0.34   0.095   0.46

    family                  y / out  gx     gW1 / gattn  gW2
    squeeze-and-excitation  0.66     0.33   0.06         0.51
    aggregate att_group     0.56     0.71   0.57
    aggregate att_mean      0.53     0.53   0.098
    aggregate mean          0.25     0.46

(g_residual is the incoming gradient itself: ratio 0.)  The one-pass and two-pass runs of a row agree bit for bit, so their
columns differ only through the rows each form takes.  No output came near 1, so neither intrinsic allowance of norm_ref.py
(RSQRT_ULPS, EXP_ULPS, 2 ulp each) had to grow (the eval-mode BatchNorm rows are part of the two-pass BatchNorm line).  Wall time of this file on
an MI355X: 8 s (tests/test_ltae_reference_gpu.py in the same visit: 139 s).

Found while writing these rows: the full-segment branches of the two-pass kernels of csrc/norm.hip and the float4 branches
of csrc/se.hip dereferenced an f32x4 (16-byte aligned type) at row bases that are only 4-byte aligned whenever HW > 2048
and HW % 4 != 0 (47 x 47 planes).  The hardware takes a 16-byte global access at any 4-byte boundary and the compiler emitted
exactly that, but the source promised an alignment it did not have; those accesses now go through f32x4u (aligned(4)), which
compiles to the same instructions.  And a real miss: se_c1024_prior put the input gradient of squeeze-and-excitation at a
Frobenius error of 5.4e-6 (bar 5e-6).  The gate kernels of csrc/se.hip summed their dot products over up to 1024 channels
sequentially in float, although the file's header promises double accumulation in the per-frame stage; an emulation of that
one sum on the CPU reproduces 5.3e-6, every other rounding of the op together 3.9e-7.  The four dot products of the gate and
its adjoint now accumulate in double.
"""
import ctypes

import pytest
import torch

import norm_ref as R
from norm_ref import assert_within

pytestmark = pytest.mark.gpu

OBSERVED = {}
REACHED_ONEPASS = set()
REACHED_BRANCHES = set()
_SHARED = {}


def _engine():
    from crop2seg_amd import engine as E
    from crop2seg_amd import _lib
    return E, _lib


def cus():
    _, L = _engine()
    n = L.lib().c2s_device_cus()
    return n if n > 0 else 256


def shared_ws():
    """One workspace for every normalisation run of this file: its sync area serves launches of every shape of the table."""
    E, _ = _engine()
    if "ws" not in _SHARED:
        _SHARED["ws"] = E.Workspace(torch.device("cuda"))
    return _SHARED["ws"]


def make_ctx(params, buffers=None, training=True, ws=None, trainable=None):
    E, _ = _engine()
    dev = torch.device("cuda")
    p = {k: v.to(dev).contiguous() for k, v in params.items()}
    b = {k: v.to(dev).contiguous() for k, v in (buffers or {}).items()}
    g = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    return E.Ctx(p, b, g, ws or E.Workspace(dev), training, E.Tape(), trainable=trainable)


def observe(family, name, ratio):
    OBSERVED[(family, name)] = max(OBSERVED.get((family, name), 0.0), ratio)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


# ------------------------------------------------------------------------------------------------ normalisation
def run_norm(row, t, onepass, side, monkeypatch):
    E, L = _engine()
    monkeypatch.setattr(E, "ONEPASS_NORM", onepass)
    monkeypatch.setattr(E, "ONEPASS_MIN_HW", 256)
    monkeypatch.setattr(E, "SIDE_WGRAD", side)
    C = row["C"]
    affine, frozen, batch = row.get("affine", True), row.get("frozen", False), row["kind"] == "batch"
    params = {"cb": torch.zeros(C)}
    if affine:
        params.update({"n.weight": t["gamma"], "n.bias": t["beta"]})
    buffers = {"n.running_mean": t["rm"].clone(), "n.running_var": t["rv"].clone(),
               "n.num_batches_tracked": torch.zeros((), dtype=torch.int64)} if batch else {}
    ctx = make_ctx(params, buffers, row.get("training", True), shared_ws(), ["n.weight", "n.bias"] if frozen else None)
    xd = t["x"].cuda()
    rd = t["res"].cuda() if t["res"] is not None else None
    vd = t["valid"].int().cuda() if not bool(t["valid"].all()) else None
    out = E.norm_act(ctx, xd, "n", L.NORM_BATCH if batch else L.NORM_GROUP, row["groups"], row.get("relu", True), rd, vd,
                     row.get("pad_value", 0.0), conv_bias=None if frozen else "cb", affine=affine)
    saved = ctx.tape.ops[-1].saved
    res = {"y": out.clone(), "group_stats": saved["group_stats"].clone(), "row_ab": saved["row_ab"].clone()}
    ctx.tape.grads[out.data_ptr()] = t["gout"].cuda().clone()
    ctx.tape.backward()
    torch.cuda.synchronize()
    assert ctx.ws.sync_error() == 0, "a one-pass normalisation wait gave up"
    gx = ctx.tape.grads.get(xd.data_ptr())
    if frozen:
        assert gx is None, "a frozen producer gets no input gradient"
    else:
        res["gx"] = gx
        res["dbias"] = ctx.g["cb"]
    if affine:
        res["dgamma"], res["dbeta"] = ctx.g["n.weight"], ctx.g["n.bias"]
    if rd is not None and not frozen:
        res["g_residual"] = ctx.tape.grads[rd.data_ptr()]
    if batch:
        res["running_mean"], res["running_var"] = ctx.b["n.running_mean"], ctx.b["n.running_var"]
        res["nbt"] = int(ctx.b["n.num_batches_tracked"])
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.items()}


def check_norm(row, t, got, o, A, family):
    keep = t["valid"]
    pad = ~keep
    batch, training = row["kind"] == "batch", row.get("training", True)
    n, C, G = int(keep.sum()), row["C"], row["groups"]
    for k in ("y", "gx", "dgamma", "dbeta", "dbias", "g_residual", "running_mean", "running_var"):
        if k not in got:
            continue
        if k in ("running_mean", "running_var") and not training:
            assert same_bits(got[k], t["rm" if k == "running_mean" else "rv"]), f"eval mode changed {k}"
            continue
        g = got[k]
        if k != "g_residual":                      # the residual branch takes g itself, padded frames and all
            assert bool(torch.isfinite(g).all()), f"{k}: non-finite values (a padded frame was read?)"
        if g.dim() == 4:
            g = g[keep]
        observe(family, k, assert_within(f"{row['name']} {k}", g, o[k], A[k], R.C_BOUND, R.norm_frob(row, k)))
    gs = got["group_stats"].view(C, 2) if batch else got["group_stats"].view(row["N"], G, 2)
    assert bool(torch.isfinite(gs).all())
    observe(family, "group_stats", assert_within(f"{row['name']} group_stats", gs if batch else gs[keep], o["group_stats"],
                                                 A["group_stats"], R.C_BOUND, R.norm_frob(row, "group_stats")))
    # row_ab of a real frame: (gamma rstd, beta, mean) of the row's channel and group
    ab = got["row_ab"].view(row["N"], C, 3)[keep].double()
    gsr, gsA = (v if batch else v.repeat_interleave(C // G, dim=1) for v in (o["group_stats"], A["group_stats"]))
    gsr, gsA = (v.expand(n, C, 2) for v in (gsr, gsA))
    gam = torch.ones(C, dtype=torch.float64) if t["gamma"] is None else t["gamma"].double()
    bet = torch.zeros(C, dtype=torch.float64) if t["beta"] is None else t["beta"].double()
    ab_ref = torch.stack([gam * gsr[..., 1], bet.expand(n, C), gsr[..., 0]], -1)
    ab_A = torch.stack([gam.abs() * (gsA[..., 1] + gsr[..., 1]), torch.zeros(n, C, dtype=torch.float64), gsA[..., 0]], -1)
    observe(family, "row_ab", assert_within(f"{row['name']} row_ab", ab, ab_ref, ab_A, R.C_BOUND, R.norm_frob(row, "group_stats")))
    if bool(pad.any()):
        pv = row.get("pad_value", 0.0)
        assert bool((got["y"][pad] == pv).all()), "y of a padded frame is not pad_value"
        if "gx" in got:
            assert bool((bits(got["gx"][pad]) == 0).all()), "gradient of a padded frame is not 0"
        assert bool((got["row_ab"].view(row["N"], C, 3)[pad] == 0).all()), "row_ab of a padded frame is not 0"
        if not batch:
            assert bool((gs[pad] == 0).all()), "group_stats of a padded GroupNorm frame is not 0"
    if batch:
        assert got["nbt"] == (1 if training else 0), "num_batches_tracked"


NORM_NAMES = [r["name"] for r in R.norm_rows(256)]


@pytest.mark.parametrize("name", NORM_NAMES)
def test_norm_rows_per_element(name, monkeypatch):
    E, L = _engine()
    row = next(r for r in R.norm_rows(cus()) if r["name"] == name)
    t = R.norm_inputs(row)
    o, A = R.norm_row_ref(row, t)
    batch = row["kind"] == "batch"
    HW = row["H"] * row["W"]
    d = L.NormDesc(row["N"], row["C"], HW, L.NORM_BATCH if batch else L.NORM_GROUP, 1 if batch else row["groups"],
                   1 if (row.get("training", True) or not batch) else 0, 1e-5, 0.1)
    has_valid = 0 if bool(t["valid"].all()) else 1
    nk = R.onepass_instance(row)
    took = L.lib().c2s_norm_onepass_sync_bytes(ctypes.byref(d), has_valid) != 0
    assert took == (nk != 0), f"{name}: one-pass form {'taken' if took else 'not taken'}, the row expects NK = {nk}"
    if "wrap" in name:
        assert (row["N"] * row["C"] * (HW // 256) + 3) // 4 >= 2.5 * 8 * cus(), "the grid of this row must wrap"
    kind = "BatchNorm" if batch else "GroupNorm"
    runs = {}
    for form, onepass, side in (("two-pass", False, True), ("two-pass, main stream", False, False)) + \
            ((("one-pass", True, True),) if nk and not row.get("frozen") else ()) + \
            ((("one-pass shape, no gx", True, True),) if nk and row.get("frozen") else ()) + \
            ((("one-pass asked, falls back", True, True),) if not nk else ()):
        got = runs[form] = run_norm(row, t, onepass, side, monkeypatch)
        check_norm(row, t, got, o, A, ("two-pass" if form.startswith("two") or not nk else "one-pass") + " " + kind)
    if nk and not row.get("frozen"):
        REACHED_ONEPASS.add((nk, bool(row.get("res")), row["kind"]))
    REACHED_BRANCHES.update(R.two_pass_branches(HW))
    first = runs["two-pass"]
    for form, got in runs.items():
        for k, v in got.items():
            if torch.is_tensor(v):
                keepf = t["valid"] if v.dim() == 4 else slice(None)
                assert same_bits(v[keepf], first[k][keepf]), f"{name}: {k} of the {form} run differs from the two-pass run"
    print(f"{name}: NK {nk}, kink rounds {t['kink_rounds']}, runs {list(runs)}")


def test_reached_instances_and_branches():
    """Closing test of the normalisation table (run after test_norm_rows_per_element in file order)."""
    want = {(nk, res, kind) for nk in (1, 2, 4, 8) for res in (False, True) for kind in ("group", "batch")}
    print("one-pass instances reached (NK, residual, kind):", sorted(REACHED_ONEPASS))
    print("two-pass branches reached:", sorted(REACHED_BRANCHES))
    assert REACHED_ONEPASS == want, sorted(want - REACHED_ONEPASS)
    assert REACHED_BRANCHES == {"scalar", "float4_tail", "full", "full_unaligned"}
    hdr = shared_ws().bufs["sync"][:16].view(torch.int32)
    assert int(hdr[0]) == 0 and int(hdr[3]) == 0, "finished-workgroup counter back at rest, no error"


# ------------------------------------------------------------------------------------------------ squeeze-and-excitation
@pytest.mark.parametrize("name", [r["name"] for r in R.se_rows()])
def test_se_rows_per_element(name):
    E, L = _engine()
    row = next(r for r in R.se_rows() if r["name"] == name)
    t = R.se_inputs(row)
    o, A = R.se_row_ref(row, t)
    wn = ["m.sae.1.weight", "m.sae.3.weight"]
    ctx = make_ctx({wn[0]: t["W1"], wn[1]: t["W2"]})
    if row.get("prior"):                           # a weight that already has a gradient: the kernel adds (acc_w1 / acc_w2)
        ctx.g[wn[0]], ctx.g[wn[1]] = t["prior_w1"].cuda(), t["prior_w2"].cuda()
        ctx._gwritten.update(wn)
    keep = t["valid"]
    pad = ~keep
    xd = t["x"].cuda()
    vd = keep.int().cuda() if bool(pad.any()) else None
    pv = row.get("pad_value", 0.0)
    out = E.squeeze_excite(ctx, xd, "m", vd, pv)
    y = out.clone().cpu()
    ctx.tape.grads[out.data_ptr()] = t["gout"].cuda().clone()
    ctx.tape.backward()
    torch.cuda.synchronize()
    gx = ctx.tape.grads[xd.data_ptr()].cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all()), "non-finite values (a padded frame was read?)"
    observe("se", "y", assert_within(f"{name} y", y[keep], o["y"], A["y"], R.C_BOUND, R.FROB["se_y"]))
    observe("se", "gx", assert_within(f"{name} gx", gx[keep], o["gx"], A["gx"], R.C_BOUND, R.FROB["se_gx"]))
    observe("se", "gW1", assert_within(f"{name} gW1", ctx.g[wn[0]], o["gW1"], A["gW1"], R.C_BOUND, R.FROB["gW1"]))
    observe("se", "gW2", assert_within(f"{name} gW2", ctx.g[wn[1]], o["gW2"], A["gW2"], R.C_BOUND, R.FROB["gW2"]))
    if bool(pad.any()):
        assert bool((y[pad] == pv).all()), "y of a padded frame is not pad_value"
        assert bool((bits(gx[pad]) == 0).all()), "gradient of a padded frame is not 0"
    print(f"{name}: kink rounds {t['kink_rounds']}, branches {sorted(R.two_pass_branches(row['H'] * row['W']))}")


# ------------------------------------------------------------------------------------------------ temporal aggregation
@pytest.mark.parametrize("name", [r["name"] for r in R.agg_rows()])
def test_agg_rows_per_element(name):
    E, L = _engine()
    row = next(r for r in R.agg_rows() if r["name"] == name)
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    mode = row.get("mode", "att_group")
    need_x, need_a = row.get("need_x", True), row.get("need_a", True)
    ctx = make_ctx({})
    x5, ad = t["x"].cuda(), t["attn"].cuda()
    keep = t["valid"]
    pad = ~keep
    vd = keep.view(-1).int().cuda() if bool(pad.any()) else None
    if not (need_x and need_a):                    # requires_grad propagation: only what is marked gets a gradient
        ctx.trainable = frozenset()
        ctx._needs.update(p.data_ptr() for p, n in ((x5, need_x), (ad, need_a)) if n)
    out = E.temporal_aggregate(ctx, x5, ad, vd, row["nh"], mode)
    got_out = out.clone().cpu()
    if t["prior_gx"] is not None:
        ctx.tape.grads[x5.data_ptr()] = t["prior_gx"].cuda().clone()
    if t["prior_gattn"] is not None:
        ctx.tape.grads[ad.data_ptr()] = t["prior_gattn"].cuda().clone()
    ctx.tape.grads[out.data_ptr()] = t["gout"].cuda().clone()
    ctx.tape.backward()
    torch.cuda.synchronize()
    fam = f"aggregate {mode}"
    observe(fam, "out", assert_within(f"{name} out", got_out, o["out"], A["out"], R.C_BOUND, R.FROB["out"]))
    gx = ctx.tape.grads.get(x5.data_ptr())
    if need_x:
        gx = gx.cpu()
        assert bool(torch.isfinite(gx).all()), "gx: non-finite values (a padded frame was read?)"
        observe(fam, "gx", assert_within(f"{name} gx", gx[keep], o["gx"][keep], A["gx"][keep], R.C_BOUND, R.FROB["agg_gx"]))
        if bool(pad.any()):
            if t["prior_gx"] is not None:
                assert same_bits(gx[pad], t["prior_gx"][pad]), "the gradient already on a padded frame was touched"
            else:
                assert bool((bits(gx[pad]) == 0).all()), "gradient of a padded frame is not 0"
    else:
        assert gx is None, "an input that needs no gradient got one"
    ga = ctx.tape.grads.get(ad.data_ptr())
    if mode == "mean" or not need_a:
        assert ga is None or t["prior_gattn"] is not None
    else:
        ga = ga.cpu()
        assert bool(torch.isfinite(ga).all()), "gattn: non-finite values (a padded frame was read?)"
        observe(fam, "gattn", assert_within(f"{name} gattn", ga[:, keep], o["gattn"][:, keep], A["gattn"][:, keep], R.C_BOUND,
                                            R.FROB["gattn"]))
        if bool(pad.any()):
            if t["prior_gattn"] is not None:
                assert same_bits(ga[:, pad], t["prior_gattn"][:, pad]), "the gradient already on a padded frame was touched"
            else:
                assert bool((bits(ga[:, pad]) == 0).all()), "attention gradient of a padded frame is not 0"


# ------------------------------------------------------------------------------------------------ dropout + per-pixel GroupNorm
@pytest.mark.parametrize("name", [r["name"] for r in R.pixel_gn_rows()])
def test_pixel_gn_rows_per_element(name):
    E, L = _engine()
    row = next(r for r in R.pixel_gn_rows() if r["name"] == name)
    t = R.pixel_gn_inputs(row)
    o, A = R.pixel_gn_row_ref(row, t)
    ctx = make_ctx({"on.weight": t["gamma"], "on.bias": t["beta"]})
    xd = t["x"].cuda()
    d = E.dropout_nchw(ctx, xd, row["p"], 0, t["keep"].cuda())
    out = E.pixel_group_norm(ctx, d, "on", row["groups"])
    y = out.clone().cpu()
    ctx.tape.grads[out.data_ptr()] = t["gout"].cuda().clone()
    ctx.tape.backward()
    torch.cuda.synchronize()
    fam = "dropout + pixel GN"
    observe(fam, "y", assert_within(f"{name} y", y, o["y"], A["y"], R.C_BOUND, R.FROB["pgn_y"]))
    observe(fam, "gx", assert_within(f"{name} gx", ctx.tape.grads[xd.data_ptr()], o["gx"], A["gx"], R.C_BOUND, R.FROB["pgn_gx"]))
    observe(fam, "dgamma", assert_within(f"{name} dgamma", ctx.g["on.weight"], o["dgamma"], A["dgamma"], R.C_BOUND, R.FROB["dgamma"]))
    observe(fam, "dbeta", assert_within(f"{name} dbeta", ctx.g["on.bias"], o["dbeta"], A["dbeta"], R.C_BOUND, R.FROB["dbeta"]))


def test_print_observed_ratios():
    """Not a check: the table of the module docstring (run with -s)."""
    fams = sorted({f for f, _ in OBSERVED})
    for f in fams:
        print(f"    {f:<24}" + "  ".join(f"{k} {v:.3g}" for (ff, k), v in sorted(OBSERVED.items()) if ff == f))
