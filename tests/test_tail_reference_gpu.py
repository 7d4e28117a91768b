"""The loss, Adam and metrics kernels (ce_*, focal_*, smooth_ce_* of csrc/loss.hip; adam_kernel of csrc/misc.hip; metrics_update,
confusion_add, boundary_target, region_relabel of csrc/metrics.hip) against the float64 references of tests/tail_ref.py,
element by element, through the public entry points: engine.cross_entropy / adam_flat, losses.focal_ce / smooth_ce /
boundary_target, metrics.StepMeters / IoU.

tests/test_tail_gpu.py and tests/test_ops_gpu.py hold these kernels to scalar-loss bars, to gradient bars relative to the
largest gradient of the tensor and to one three-step Adam run of 1000 elements; a wrong value on a low-gradient pixel, a
wrong class row or a mis-scaled Adam step passes those, and none of their inputs is large enough for a second grid pass, so
a block partial lost there passes too (test_tail_reference.py plants each).  Here every floating-point output must satisfy |got - ref| <= 2 u A (u = 2^-24, A =
first-order rounding propagation, tail_ref.py) next to the existing bars, and every integer output must match bit for bit.
The row tables are module-level: tests/test_tail_reference.py evaluates the same rows in float32 on the CPU (ratio <= 1: the
constant 2 is not fitted to the kernels) and plants its faults on them.  test_rows_reach_every_path asserts from the tables
that every grid-stride path, every K edge and every gamma ran.

Worst ratios |err| / (u A) observed on an MI355X (printed with -s; for information, the constant does not move):

    family            loss   glogits  tot    pixel_loss  |  family            m      v      p      upd
    cross entropy     0.32   0.87     0.52               |  Adam, one step    0.93   0.98   0.96   0.95
    focal CE          0.14   0.73     0.63               |  Adam, 20 steps    0.84   0.92   0.89   0.89
    focal gamma 0     0.14   0.73            (against the cross-entropy reference)
    smooth CE         0.13   0.48     0.10   0.74

The bad-target and bad-label counters, the predictions, both confusion matrices, boundary_target and region_relabel were
bit-exact.  No output came near 2 and the named terms ended where they started: EXP_ULPS = LOG_ULPS = POW_ULPS = 2 ulp.  The
cross-entropy kernels keep the fast __expf / __logf: with the same 2 ulp their rows stayed at 0.87 and below.  The 20-step Adam
run ended at a Frobenius error of p of 3.28e-07 against the float64 run from the start; one float32 step of the reference on
the same inputs errs by 1.73e-08, so the bar is 3.46e-07.  Wall time of this file on an MI355X: 1.5 s for 102 cases.

What the saturated rows require: focal_sat_g0.0, focal_sat_g0.5 and their K = 2 twins hold pixels with pt == 1.f in float32
(asserted on the CPU), where gamma (1-pt)^(gamma-1) pt log pt is inf * 0 as written; the gradient there must be finite and
within the bound of the limit, -(1-pt)^gamma (delta_kt - p_k) / n, for every gamma < 1, and for gamma = 0 equal cross entropy.

The Frobenius bar of the Adam update, tail_ref.adam_upd_frob, holds three terms: ADAM_FROB for the step arithmetic, the rounding
of the stored p' (2 u |p'| / |upd|) and C_BOUND u bc_rel, the relative error that the cancellation in 1 - b^step puts on every
element alike.  Its docstring says at which steps that makes a tight check of the step size (1000 and 100000) and at which not.
"""
import itertools

import numpy as np
import pytest
import torch

import tail_ref as R
from tail_ref import assert_within

pytestmark = pytest.mark.gpu

OBSERVED = {}
RAN = set()
_REF = {}

CE_CAP = 512 * 256            # pixels of one grid pass: ce_fwd / ce_bwd / focal_fwd / smooth_ce
FOCAL_BWD_CAP = 2048 * 256    # focal_bwd, boundary_target, region_relabel
METRICS_CAP = 1024 * 256      # metrics_update, confusion_add
ADAM_CAP = 2048 * 256
GAMMAS = (0.0, 0.5, 1.0, 2.0)
LOGIT_KINDS = ("normal", "x8", "+80", "-80", "ties", "sat")


# ------------------------------------------------------------------------------------------------ row tables
def _ce_rows():
    rows = []
    for i, (HW, K) in enumerate(itertools.product((1, 5, 63, 257), (1, 2, 15, 20, 32, 40))):
        rows.append(dict(name=f"ce_hw{HW}_k{K}", B=3, K=K, H=1, W=HW, seed=100 + i, logits=LOGIT_KINDS[i % 6],
                         ls=(0.0, 0.1, 1.0)[(i // 2) % 3], weights=(None, "rand0")[(i // 3) % 2],
                         ignore=-100 if K == 1 or (i // 5) % 2 == 0 else 0, bad=i % 4 == 1))
    rows += [
        dict(name="ce_grid", B=3, K=2, H=210, W=210, seed=150, ls=0.1, weights="rand0", bad=True),
        dict(name="ce_ignore_block", B=3, K=15, H=1, W=257, seed=151, ls=0.1, ignore_block=True),
        dict(name="ce_zero_block", B=3, K=15, H=1, W=257, seed=152, ls=0.0, weights="zero_block"),
        dict(name="ce_zero_block_ls", B=3, K=20, H=1, W=257, seed=153, ls=0.1, weights="zero_block", ignore=0, bad=True),
        dict(name="ce_sat_x_ls1", B=3, K=32, H=1, W=63, seed=154, ls=1.0, logits="sat", weights="rand0"),
    ]
    return rows


def _focal_rows():
    rows = []
    for i, (HW, K) in enumerate(itertools.product((1, 5, 63, 257), (1, 2, 15, 20, 32))):
        rows.append(dict(name=f"focal_hw{HW}_k{K}", B=3, K=K, H=1, W=HW, seed=200 + i, logits=LOGIT_KINDS[i % 6],
                         gamma=GAMMAS[i % 4], size_average=(i // 2) % 2 == 0, weights=(None, "rand0")[(i // 4) % 2],
                         ignore=-100 if K == 1 or (i // 3) % 2 == 0 else 0, bad=i % 4 == 2, prior=0.25 if i % 5 == 0 else None))
    for j, gamma in enumerate(GAMMAS):
        rows.append(dict(name=f"focal_sat_g{gamma}", B=3, K=15, H=1, W=63, seed=230 + j, logits="sat", gamma=gamma))
        rows.append(dict(name=f"focal_sat_k2_g{gamma}", B=3, K=2, H=1, W=257, seed=240 + j, logits="sat", gamma=gamma,
                         weights="rand0", size_average=j % 2 == 0, prior=-1.5 if j == 1 else None, ignore_block=True))
    rows += [
        dict(name="focal_g0_is_ce", B=3, K=20, H=1, W=257, seed=250, gamma=0.0, logits="x8"),
        dict(name="focal_fwd_grid", B=3, K=2, H=210, W=210, seed=251, gamma=2.0, weights="rand0", bad=True),
        dict(name="focal_bwd_grid", B=3, K=2, H=419, W=419, seed=252, gamma=0.5),
    ]
    return rows


def _smooth_rows():
    rows = []
    Ks = (1, 2, 15, 20, 32)
    for i, ((H, W), ls) in enumerate(itertools.product(((1, 9), (9, 1), (5, 7), (40, 36)), (0.0, 0.1, 1.0))):
        K = Ks[i % 5]
        rows.append(dict(name=f"smooth_{H}x{W}_ls{ls}_k{K}", B=3, K=K, H=H, W=W, seed=300 + i, ls=ls,
                         logits=LOGIT_KINDS[(i + 1) % 5], bg=i % 2 == 0, bg_index=0 if K < 4 or i % 4 == 0 else 3,
                         reduction=("mean", "sum", "none")[i % 3], weights=(None, "rand0")[(i // 2) % 2], bad=i % 3 == 1,
                         want_grad=i % 6 != 5, pl=i % 4 == 0))
    rows += [
        dict(name="smooth_k32_adjacent", B=3, K=32, H=1, W=9, seed=320, ls=0.1, adjacent=True),
        dict(name="smooth_k32_adjacent_col", B=3, K=32, H=9, W=1, seed=321, ls=0.1, adjacent=True, weights="rand0", bg=True,
             bg_index=31),
        dict(name="smooth_batch_edge", B=3, K=15, H=5, W=7, seed=322, ls=0.1, rows_constant=True),
        dict(name="smooth_grid", B=3, K=2, H=210, W=210, seed=323, ls=0.1, bad=True, weights="rand0"),
    ]
    return rows


def _adam_rows():
    rows = [
        dict(name="adam_n1", n=1, offset=0, step=1),
        dict(name="adam_n1_off3", n=1, offset=3, step=100000, gs=0.125),
        dict(name="adam_n255_off1", n=255, offset=1, step=2, gs=0.125),
        dict(name="adam_n255_off3", n=255, offset=3, step=100000),
        dict(name="adam_n257_off3", n=257, offset=3, step=10),
        dict(name="adam_n257_off1", n=257, offset=1, step=1000, gs=0.125),
        dict(name="adam_grid_off1", n=ADAM_CAP + 3, offset=1, step=2, gs=0.125),
        dict(name="adam_grid_off3", n=ADAM_CAP + 3, offset=3, step=1000),
        dict(name="adam_zero", n=257, offset=1, step=1, grad="zero"),
        dict(name="adam_tiny", n=257, offset=0, step=10, grad="tiny"),
        dict(name="adam_tiny_gs", n=255, offset=3, step=1, grad="tiny", gs=0.125),
        dict(name="adam_huge", n=255, offset=1, step=2, grad="huge"),
        dict(name="adam_huge_gs", n=257, offset=3, step=1000, grad="huge", gs=0.125),
    ]
    for i, r in enumerate(rows):
        r["seed"] = 400 + i
    return rows


def _metric_rows():
    rows = [dict(name=f"metrics_k{K}", B=3, K=K, H=5, W=7, seed=500 + i) for i, K in enumerate((1, 2, 15, 32))]
    rows += [dict(name="metrics_k15_blocks", B=3, K=15, H=23, W=19, seed=510),
             dict(name="metrics_grid", B=3, K=2, H=296, W=296, seed=511)]
    return rows


BOUNDARY_ROWS = [
    dict(name="boundary_1x1x5", B=1, H=1, W=5, seed=600),
    dict(name="boundary_2x5x1", B=2, H=5, W=1, seed=601),
    dict(name="boundary_2x12x17", B=2, H=12, W=17, seed=602),
    dict(name="boundary_grid", B=2, H=513, W=512, seed=603),
]
CE_ROWS, FOCAL_ROWS, SMOOTH_ROWS, ADAM_ROWS, METRIC_ROWS = _ce_rows(), _focal_rows(), _smooth_rows(), _adam_rows(), _metric_rows()
CE_ALL_IGNORED = dict(name="ce_all_ignored", B=3, K=15, H=1, W=63, seed=160, ls=0.1, all_ignored=True)


def ids(rows):
    return [r["name"] for r in rows]


# ------------------------------------------------------------------------------------------------ inputs and references
def ce_args(row):
    z, t, cw = R.make_loss_inputs(row)
    return z, t, dict(class_w=cw, label_smoothing=row.get("ls", 0.0), ignore_index=row.get("ignore", -100))


def focal_args(row):
    z, t, cw = R.make_loss_inputs(row)
    prior = None if row.get("prior") is None else torch.tensor([row["prior"]], dtype=torch.float32)
    return z, t, dict(gamma=row["gamma"], ignore_index=row.get("ignore", -100), class_w=cw,
                      size_average=row.get("size_average", True), prior=prior)


def smooth_args(row):
    z, t, cw = R.make_loss_inputs(dict(row, ignore=None))       # this loss has no ignore_index
    B, K, H, W = z.shape
    if row.get("adjacent"):                                     # classes 30 and 31 side by side: bits 30 and 31 of the mask
        tf = t.reshape(B, -1)
        tf[:, 0], tf[:, 1], tf[:, 2] = 30, 31, 31
    if row.get("rows_constant"):                                # the last row of an entry and the first of the next differ
        for b in range(B):
            t[b] = (b * 4 + torch.arange(H)[:, None] // 2) % K
    bg = None
    if row.get("bg"):
        gen = torch.Generator().manual_seed(row["seed"] + 1000)
        bg = torch.rand(K, generator=gen) + 0.05
        bg = (bg / bg.sum()).float()
    return z, t, dict(label_smoothing=row["ls"], class_w=cw, bg=bg, bg_index=row.get("bg_index", 0),
                      reduction=row.get("reduction", "mean"))


def adam_kwargs(row):
    return dict(step=row["step"], grad_scale=row.get("gs", 1.0))


def reference(kind, row):
    """The float64 reference of a row, computed once and shared."""
    key = (kind, row["name"])
    if key not in _REF:
        if kind == "adam":
            p, g, m, v, off, n = R.make_adam_inputs(row)
            s = slice(off, off + n)
            _REF[key] = R.adam_ref(p[s], g[s], m[s], v[s], **adam_kwargs(row))
        else:
            z, t, kw = {"ce": ce_args, "focal": focal_args, "smooth": smooth_args}[kind](row)
            _REF[key] = {"ce": R.ce_ref, "focal": R.focal_ref, "smooth": R.smooth_ref}[kind](z, t, **kw)
    return _REF[key]


def make_metric_inputs(row, call):
    """Logits [B,K,H,W] and targets [B,H,W] of update call `call` of a metrics row: halves (ties for first and second place),
    the first pixels with NaN in the first / a middle / the last class, two NaN, +inf, -inf everywhere but one class, all
    equal, +inf next to NaN; every third target the second choice; targets K, -1 and -100."""
    B, K, H, W = row["B"], row["K"], row["H"], row["W"]
    gen = torch.Generator().manual_seed(row["seed"] + 50 * call)
    z = torch.round(torch.randn(B, K, H, W, generator=gen) * 2) / 2
    zr = z.reshape(B, K, -1)
    mid, nan, inf = K // 2, float("nan"), float("inf")
    for b in range(B):
        zr[b, 0, 0] = nan
        zr[b, mid, 1] = nan
        zr[b, K - 1, 2] = nan
        zr[b, 0, 3], zr[b, K - 1, 3] = nan, nan
        zr[b, mid, 4] = inf
        zr[b, :, 5] = -inf
        zr[b, (b + 1) % K, 5] = -3.0
        zr[b, :, 6] = 1.5
        zr[b, 0, 7], zr[b, K - 1, 7] = inf, nan
        zr[b, :, 8] = -inf
        zr[b, :, 9] = inf
    t = torch.randint(0, K, (B, H, W), generator=gen)
    tf = t.reshape(-1)
    _, second = R.metrics_scan(z)
    tf[::3] = torch.from_numpy(second)[::3]
    n = tf.numel()
    for i, val in zip((10, n // 2, n - 2, n - 1), (K, -1, -100, K + 5)):
        tf[i] = val
    return z, t


def make_labels(row, K=4):
    B, H, W = row["B"], row["H"], row["W"]
    gen = torch.Generator().manual_seed(row["seed"])
    y = torch.randint(0, K, (B, max(1, H // 3 + 1), max(1, W // 3 + 1)), generator=gen)
    y = y.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W].contiguous()        # 3 x 3 fields: interiors exist
    noise = torch.rand(B, H, W, generator=gen) < 0.05
    return torch.where(noise, torch.randint(0, K, (B, H, W), generator=gen), y)


# ------------------------------------------------------------------------------------------------ helpers
def _engine():
    from crop2seg_amd import engine as E
    from crop2seg_amd import _lib
    return E, _lib


def dev():
    return torch.device("cuda")


def observe(family, name, ratio):
    OBSERVED[(family, name)] = max(OBSERVED.get((family, name), 0.0), ratio)
    print(f"  {family:8s} {name:10s} ratio {ratio:.3f}")


def check(family, name, got, ref, A, frob, max_rel=None):
    got = got.detach().double().cpu().reshape(ref[name].shape)
    if max_rel is not None:
        err, top = float((got - ref[name]).abs().max()), float(ref[name].abs().max())
        print(f"  {family:8s} {name:10s} max err {err:.3e} of max {top:.3e}")
        assert err <= max_rel * top, f"{family} {name}: max error {err:.3e} > {max_rel:g} * {top:.3e}"
    observe(family, name, assert_within(f"{family} {name}", got, ref[name], A[name], R.C_BOUND, frob))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("row", CE_ROWS, ids=ids(CE_ROWS))
def test_cross_entropy(row):
    E, _ = _engine()
    z, t, kw = ce_args(row)
    ref, A = reference("ce", row)
    cw = torch.ones(row["K"]) if kw["class_w"] is None else kw["class_w"]
    ws = E.Workspace(dev())
    zd, td, cd = z.cuda(), t.cuda(), cw.cuda()
    loss, gl = E.cross_entropy(zd, td, cd, ws, True, kw["label_smoothing"], kw["ignore_index"])
    tail = ws.bufs["ce"][-3:].clone()
    check("ce", "loss", loss, ref, A, R.SCALAR_REL)
    check("ce", "glogits", gl, ref, A, 1e-5, R.GRAD_MAX_REL)
    check("ce", "tot", tail[:2], ref, A, R.SCALAR_REL)
    check("ce", "bad", tail[2:], ref, A, R.SCALAR_REL)
    assert E.bad_target_count(ws) == int(ref["bad"])
    loss2, none = E.cross_entropy(zd, td, cd, ws, False, kw["label_smoothing"], kw["ignore_index"])
    assert none is None and bool((bits(loss2) == bits(loss)).all()), "the forward-only call gives another loss"
    RAN.add(row["name"])


def test_cross_entropy_all_ignored():
    """No kept pixel: the weight sum is 0, the loss 0 / 0 = NaN (torch gives NaN too), every gradient element exactly 0."""
    E, _ = _engine()
    z, t, kw = ce_args(CE_ALL_IGNORED)
    ws = E.Workspace(dev())
    loss, gl = E.cross_entropy(z.cuda(), t.cuda(), torch.ones(15).cuda(), ws, True, kw["label_smoothing"], kw["ignore_index"])
    assert bool(torch.isnan(loss).all())
    assert bool((bits(gl) == 0).all())
    assert E.bad_target_count(ws) == 0 and ws.bufs["ce"][-3:].tolist()[:2] == [0.0, 0.0]
    RAN.add(CE_ALL_IGNORED["name"])


# ------------------------------------------------------------------------------------------------ focal CE
@pytest.mark.parametrize("row", FOCAL_ROWS, ids=ids(FOCAL_ROWS))
def test_focal_ce(row):
    E, _ = _engine()
    from crop2seg_amd.learning import losses
    z, t, kw = focal_args(row)
    ref, A = reference("focal", row)
    ws = E.Workspace(dev())
    prior = None if kw["prior"] is None else kw["prior"].cuda()
    cw = None if kw["class_w"] is None else kw["class_w"].cuda()
    loss, gl = losses.focal_ce(z.cuda(), t.cuda(), kw["gamma"], kw["ignore_index"], True, ws, prior, cw, kw["size_average"])
    assert prior is None or loss.data_ptr() == prior.data_ptr()
    tail = ws.bufs["focal"][-4:-1].clone()
    check("focal", "loss", loss, ref, A, R.SCALAR_REL)
    check("focal", "glogits", gl, ref, A, 1e-5, R.GRAD_MAX_REL)
    check("focal", "tot", tail, ref, A, R.SCALAR_REL)
    loss2, none = losses.focal_ce(z.cuda(), t.cuda(), kw["gamma"], kw["ignore_index"], False, ws, None, cw, kw["size_average"])
    assert none is None
    if prior is None:
        assert bool((bits(loss2) == bits(loss)).all()), "the forward-only call gives another loss"
    if row["gamma"] == 0.0 and cw is None and kw["size_average"] and prior is None:
        # gamma = 0 is plain cross entropy: the same kernel outputs against the CE reference, within the focal bound
        cref, _ = R.ce_ref(z, t, None, 0.0, kw["ignore_index"])
        for name, got in (("loss", loss), ("glogits", gl)):
            got = got.detach().double().cpu().reshape(ref[name].shape)
            observe("focal=ce", name, assert_within(f"focal gamma 0 vs CE {name}", got, cref[name], A[name], R.C_BOUND, 1e-5))
    RAN.add(row["name"])


# ------------------------------------------------------------------------------------------------ smooth CE
@pytest.mark.parametrize("row", SMOOTH_ROWS, ids=ids(SMOOTH_ROWS))
def test_smooth_ce(row):
    E, _ = _engine()
    from crop2seg_amd.learning import losses
    z, t, kw = smooth_args(row)
    ref, A = reference("smooth", row)
    ws = E.Workspace(dev())
    want_grad = row.get("want_grad", True)
    want_pl = kw["reduction"] == "none" or row.get("pl", False)
    pl = torch.full(t.shape, float("nan"), device=dev()) if want_pl else None
    cw = None if kw["class_w"] is None else kw["class_w"].cuda()
    bg = None if kw["bg"] is None else kw["bg"].cuda()
    loss, gl, counters = losses.smooth_ce(z.cuda(), t.cuda(), kw["label_smoothing"], cw, bg, kw["bg_index"], want_grad, ws,
                                          None, kw["reduction"], pl)
    check("smooth", "loss", loss, ref, A, R.SCALAR_REL)
    check("smooth", "tot", counters, ref, A, R.SCALAR_REL)
    if want_pl:
        check("smooth", "pixel_loss", pl, ref, A, 4e-6, 4e-6)
    if want_grad:
        check("smooth", "glogits", gl, ref, A, 1e-5, 2e-6)
    else:
        assert gl is None
    RAN.add(row["name"])


# ------------------------------------------------------------------------------------------------ Adam
def run_adam(row, use_step_dev):
    E, _ = _engine()
    p, g, m, v, off, n = R.make_adam_inputs(row)
    pd, gd, md, vd = p.cuda(), g.cuda(), m.cuda(), v.cuda()
    s = slice(off, off + n)
    kw = adam_kwargs(row)
    sd = torch.tensor([kw["step"]], dtype=torch.int32, device=dev()) if use_step_dev else None
    E.adam_flat(pd[s], gd[s], md[s], vd[s], 0 if use_step_dev else kw["step"], grad_scale=kw["grad_scale"], step_dev=sd)
    torch.cuda.synchronize()
    return (p, g, m, v), (pd.cpu(), gd.cpu(), md.cpu(), vd.cpu()), s


@pytest.mark.parametrize("row", ADAM_ROWS, ids=ids(ADAM_ROWS))
def test_adam(row):
    ref, A = reference("adam", row)
    (p, g, m, v), (pn, gn, mn, vn), s = run_adam(row, False)
    outside = torch.ones(p.numel(), dtype=torch.bool)
    outside[s] = False
    for name, before, after in (("p", p, pn), ("g", g, gn), ("m", m, mn), ("v", v, vn)):
        assert bool((bits(before)[outside] == bits(after)[outside]).all()), f"{name} changed outside the slice"
    assert bool((bits(g) == bits(gn)).all())
    check("adam", "m", mn[s], ref, A, R.ADAM_FROB)
    check("adam", "v", vn[s], ref, A, R.ADAM_FROB)
    check("adam", "p", pn[s], ref, A, R.ADAM_FROB)
    upd = pn[s].double() - p[s].double()                     # the update on its own
    check("adam", "upd", upd, ref, A, R.adam_upd_frob(ref, A))
    if row.get("grad") == "zero":
        assert bool((bits(pn) == bits(p)).all()) and bool((mn == 0).all()) and bool((vn == 0).all())
    _, (p2, _, m2, v2), _ = run_adam(row, True)
    for name, a, b in (("p", pn, p2), ("m", mn, m2), ("v", vn, v2)):
        assert bool((bits(a) == bits(b)).all()), f"{name}: the device step counter gives other bits than the host one"
    RAN.add(row["name"])


def adam_run_inputs():
    gen = torch.Generator().manual_seed(450)
    n = 1000
    return torch.randn(n, generator=gen) * 1e-2, [torch.randn(n, generator=gen) for _ in range(20)]


def adam_run_reference():
    """(p after 20 float64 steps from the start, Frobenius error of ONE float32 step on the same inputs)."""
    p0, grads = adam_run_inputs()
    p, m, v = p0.double(), torch.zeros(1000, dtype=torch.float64), torch.zeros(1000, dtype=torch.float64)
    for i, g in enumerate(grads):
        o, _ = R.adam_ref(p, g, m, v, i + 1, bounds=False)
        p, m, v = o["p"], o["m"], o["v"]
    z = torch.zeros(1000)
    o64, _ = R.adam_ref(p0, grads[0], z, z, 1, bounds=False)
    o32, _ = R.adam_ref(p0, grads[0], z, z, 1, dtype=torch.float32)
    single = float((o32["p"].double() - o64["p"]).norm() / o64["p"].norm())
    return p, single


def test_adam_twenty_steps():
    """Every step against the reference restarted from the kernel's own previous state (single-step bounds), then p against a
    float64 run from the start: at most 20 x the Frobenius error of one float32 step of the reference on the same inputs."""
    E, _ = _engine()
    p0, grads = adam_run_inputs()
    pd, md, vd = p0.cuda(), torch.zeros(1000, device=dev()), torch.zeros(1000, device=dev())
    for i, g in enumerate(grads):
        before = (pd.cpu(), md.cpu(), vd.cpu())
        E.adam_flat(pd, g.cuda(), md, vd, i + 1)
        ref, A = R.adam_ref(before[0], g, before[1], before[2], i + 1)
        for name, got in (("m", md), ("v", vd), ("p", pd)):
            observe("adam20", name, assert_within(f"step {i + 1} {name}", got, ref[name], A[name], R.C_BOUND, R.ADAM_FROB))
        upd = pd.cpu().double() - before[0].double()
        observe("adam20", "upd", assert_within(f"step {i + 1} upd", upd, ref["upd"], A["upd"], R.C_BOUND,
                                                       R.adam_upd_frob(ref, A)))
    p64, single = adam_run_reference()
    fr = float((pd.cpu().double() - p64).norm() / p64.norm())
    print(f"  adam 20 steps: Frobenius error of p {fr:.3e}; one float32 step of the reference {single:.3e} (bar {20 * single:.3e})")
    assert fr <= 20 * single
    RAN.add("adam_twenty_steps")


# ------------------------------------------------------------------------------------------------ metrics and labels
@pytest.mark.parametrize("row", METRIC_ROWS, ids=ids(METRIC_ROWS))
def test_metrics_update(row):
    from crop2seg_amd.learning import metrics
    K = row["K"]
    meters = metrics.StepMeters(K, device=dev())
    iou = metrics.IoU(K, cm_device=dev())
    iou_idx = metrics.IoU(K, cm_device=dev())
    conf = conf2 = conf_idx = None
    for call in range(2):
        z, t = make_metric_inputs(row, call)
        pred, top2, conf, conf2 = R.metrics_ref(z, t, conf, conf2)
        got = meters.update(z.cuda(), t.cuda(), want_pred=call == 0)
        if call == 0:
            assert np.array_equal(got[0].cpu().numpy(), pred) and np.array_equal(got[1].cpu().numpy(), top2)
        else:
            assert got is None
        iou.add(z.cuda(), t.cuda())                                 # no top-2 matrix, no prediction outputs
        wild = torch.from_numpy(pred).clone()                       # class-index predictions, some outside [0, K)
        wild.reshape(-1)[::7] = K
        wild.reshape(-1)[3::11] = -2
        conf_idx = R.confusion_add_ref(wild, t, K, conf_idx)
        iou_idx.add(wild.cuda(), t.cuda())
        assert np.array_equal(meters.iou.conf_metric.conf.cpu().numpy(), conf), f"top-1 matrix after call {call + 1}"
        assert np.array_equal(meters.iou_top2.conf_metric.conf.cpu().numpy(), conf2), f"top-2 matrix after call {call + 1}"
        assert np.array_equal(iou.conf_metric.conf.cpu().numpy(), conf)
        assert np.array_equal(iou_idx.conf_metric.conf.cpu().numpy(), conf_idx)
    RAN.add(row["name"])


@pytest.mark.parametrize("row", BOUNDARY_ROWS, ids=ids(BOUNDARY_ROWS))
def test_boundary_and_region(row):
    _, L = _engine()
    from crop2seg_amd.learning import losses, metrics
    y = make_labels(row)
    yd = y.cuda()
    assert np.array_equal(losses.boundary_target(yd).cpu().numpy(), R.boundary_target_ref(y))
    for region, keep in (("boundary", 1), ("interior", 0)):
        meters = metrics.StepMeters(4, ignore_index=-1, device=dev(), test_region=region)
        assert np.array_equal(meters.region_target(yd).cpu().numpy(), R.region_relabel_ref(y, keep, 3))
        out = torch.empty_like(yd)                                  # a negative ignore label: the export itself
        B, H, W = y.shape
        L.check(L.lib().c2s_region_relabel(yd.data_ptr(), out.data_ptr(), B, H, W, keep, -100,
                                           torch.cuda.current_stream().cuda_stream), "region_relabel")
        assert np.array_equal(out.cpu().numpy(), R.region_relabel_ref(y, keep, -100))
    RAN.add(row["name"])


# ------------------------------------------------------------------------------------------------ closing
def table_coverage():
    """What the row tables reach, from the tables alone (also asserted on the CPU by test_tail_reference.py)."""
    px = lambda r: r["B"] * r["H"] * r["W"]      # noqa: E731
    return {
        "ce_grid": [r["name"] for r in CE_ROWS if px(r) > CE_CAP],
        "focal_fwd_grid": [r["name"] for r in FOCAL_ROWS if px(r) > CE_CAP],
        "focal_bwd_grid": [r["name"] for r in FOCAL_ROWS if px(r) > FOCAL_BWD_CAP and r["W"] % 4 != 0],
        "smooth_grid": [r["name"] for r in SMOOTH_ROWS if px(r) > CE_CAP],
        "metrics_grid": [r["name"] for r in METRIC_ROWS if px(r) > METRICS_CAP],
        "adam_grid": [r["name"] for r in ADAM_ROWS if r["n"] > ADAM_CAP],
        "boundary_grid": [r["name"] for r in BOUNDARY_ROWS if px(r) > FOCAL_BWD_CAP],
        "ce_K": sorted({r["K"] for r in CE_ROWS}),
        "focal_K": sorted({r["K"] for r in FOCAL_ROWS}),
        "smooth_K": sorted({r["K"] for r in SMOOTH_ROWS}),
        "metrics_K": sorted({r["K"] for r in METRIC_ROWS}),
        "gammas": sorted({r["gamma"] for r in FOCAL_ROWS}),
        "sat_gammas": sorted({r["gamma"] for r in FOCAL_ROWS if r.get("logits") == "sat"}),
        "ce_ls": sorted({r.get("ls", 0.0) for r in CE_ROWS}),
        "smooth_ls": sorted({r["ls"] for r in SMOOTH_ROWS}),
        "smooth_hw": sorted({(r["H"], r["W"]) for r in SMOOTH_ROWS}),
        "smooth_reductions": sorted({r.get("reduction", "mean") for r in SMOOTH_ROWS}),
        "adam_steps": sorted({r["step"] for r in ADAM_ROWS}),
        "adam_offsets": sorted({r["offset"] for r in ADAM_ROWS}),
        "adam_n": sorted({r["n"] for r in ADAM_ROWS}),
    }


def assert_table_coverage():
    c = table_coverage()
    for k in ("ce_grid", "focal_fwd_grid", "focal_bwd_grid", "smooth_grid", "metrics_grid", "adam_grid", "boundary_grid"):
        assert c[k], f"no row past the grid cap: {k}"
    assert c["ce_K"] == [1, 2, 15, 20, 32, 40] and c["focal_K"] == [1, 2, 15, 20, 32] == c["smooth_K"]
    assert c["metrics_K"] == [1, 2, 15, 32]
    assert c["gammas"] == list(GAMMAS) == c["sat_gammas"]
    assert c["ce_ls"] == [0.0, 0.1, 1.0] == c["smooth_ls"]
    assert c["smooth_hw"] == [(1, 9), (5, 7), (9, 1), (40, 36), (210, 210)]
    assert c["smooth_reductions"] == ["mean", "none", "sum"]
    assert c["adam_steps"] == [1, 2, 10, 1000, 100000] and c["adam_offsets"] == [0, 1, 3]
    assert c["adam_n"] == [1, 255, 257, ADAM_CAP + 3]


def test_rows_reach_every_path():
    """Every row of every table ran (and passed), and the tables hold every grid-stride row, K edge, gamma and step."""
    assert_table_coverage()
    names = {r["name"] for rows in (CE_ROWS, FOCAL_ROWS, SMOOTH_ROWS, ADAM_ROWS, METRIC_ROWS, BOUNDARY_ROWS) for r in rows}
    names |= {CE_ALL_IGNORED["name"], "adam_twenty_steps"}
    assert names <= RAN, f"rows that did not run or did not pass: {sorted(names - RAN)}"
    worst = {}
    for (family, name), r in OBSERVED.items():
        worst.setdefault(family, {})[name] = r
    for family in sorted(worst):
        print(f"  worst ratio |err| / (u A)  {family:9s} " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(worst[family].items())))
