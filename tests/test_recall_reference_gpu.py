"""RecallCrossEntropy on the device (csrc/loss.hip) against the float64 reference of tests/recall_ref.py, through the public
entry points losses.recall_ce / losses.RecallCrossEntropy, and TrainStep(criterion=...) with each of the three criteria of
learning/losses.py.

Counts, the bad-label count and the weights must match bit for bit; the loss, every gradient element, the per-pixel nll of
the workspace and the total must satisfy |got - ref| <= 2 u A (u = 2^-24, A = first-order rounding propagation,
recall_ref.py) next to the scalar and max-relative bars of tail_ref.  The row table is module-level:
tests/test_recall_reference.py evaluates the same rows in float32 on the CPU (ratio <= 1: the constant 2 is not fitted to the
kernels) and plants its faults on them.  Every row whose pixel count is no multiple of 256 (all but `aligned`) runs inside
the guard-band arena of tests/redzone.py, as test_redzone_gpu.in_arena does: guard bands intact, no poison left in an
output.

Worst ratios |err| / (u A) observed on an MI355X (printed with -s; for information, the constant does not move):

    family            loss   glogits  nll    tot
    recall CE         0.48   0.77     0.74   0.46

Counts, bad-label counts and weights were bit-exact on every row, two consecutive calls gave the same bits, and every TrainStep
identity below held bit for bit.
"""
import itertools

import numpy as np
import pytest
import torch

import recall_ref as RR
import tail_ref as R
from tail_ref import assert_within

pytestmark = pytest.mark.gpu

OBSERVED = {}
RAN = set()
_REF = {}

RECALL_COUNT_CAP = 512 * 256      # pixels of one grid pass of recall_count_kernel
RECALL_LOSS_CAP = 512 * 256       # recall_loss_kernel
RECALL_BWD_CAP = 512 * 256        # recall_bwd_kernel
LOGIT_KINDS = ("normal", "x8", "+80", "-80", "ties", "sat")
IGNORES = (None, -1, -100, 255, 0)          # None: no ignored pixel present (the call still passes 255); 0: a real class


# ------------------------------------------------------------------------------------------------ row table
def _rows():
    rows = []
    for i, (HW, K) in enumerate(itertools.product((1, 5, 63, 257), (1, 2, 15, 20, 32))):
        ign = IGNORES[(i + i // 5) % 5]
        rows.append(dict(name=f"recall_hw{HW}_k{K}", B=3, K=K, H=1, W=HW, seed=700 + i, logits=LOGIT_KINDS[i % 6],
                         ignore=ign, bad=(i // 5) % 2 == 1))
    rows += [
        dict(name="perfect", B=3, K=15, H=1, W=63, seed=730, ignore=None, special="perfect"),
        dict(name="all_wrong", B=3, K=15, H=1, W=63, seed=731, ignore=-1, special="all_wrong"),
        dict(name="one_class", B=3, K=20, H=1, W=63, seed=732, ignore=None, special="one_class"),
        dict(name="all_ignored", B=3, K=15, H=1, W=63, seed=733, ignore=-1, all_ignored=True),
        dict(name="class1_perfect_with_ignored", B=3, K=5, H=1, W=63, seed=734, ignore=-1, special="class1_perfect"),
        dict(name="ties_k2", B=3, K=2, H=1, W=257, seed=735, logits="ties", ignore=-100, bad=True),
        dict(name="aligned", B=2, K=15, H=16, W=16, seed=736, ignore=255, bad=True),
        dict(name="recall_grid", B=3, K=2, H=210, W=210, seed=737, ignore=-1, bad=True),
    ]
    return rows


ROWS = _rows()


def ids(rows):
    return [r["name"] for r in rows]


def pixels(row):
    return row["B"] * row["H"] * row["W"]


def ignore_index(row):
    return 255 if row["ignore"] is None else row["ignore"]


def make_inputs(row):
    """Logits [B,K,H,W] float32 and targets [B,H,W] int64 of a row: tail_ref.make_loss_inputs (a fifth of the pixels on the
    ignore label unless the row has none, labels K and -7 with `bad`), then the named constructions."""
    z, t, _ = R.make_loss_inputs(row)
    B, K = z.shape[:2]
    zr = z.reshape(B, K, -1).permute(0, 2, 1).reshape(-1, K)
    tf = t.reshape(-1)
    kind = row.get("special")
    if kind == "perfect":
        tf[:] = zr.argmax(1)
    elif kind == "all_wrong":
        keep = tf != row["ignore"]
        tf[keep] = ((zr.argmax(1) + 1) % K)[keep]
    elif kind == "one_class":
        tf[:] = 3
    elif kind == "class1_perfect":
        tf[::4] = 1
        tf[2::8] = row["ignore"]
        zr = zr.clone()
        zr[tf == 1, 1] += 30.0
        z = zr.reshape(B, -1, K).permute(0, 2, 1).reshape(z.shape).contiguous()
    return z, t


def reference(row):
    """The float64 reference of a row, computed once and shared."""
    if row["name"] not in _REF:
        z, t = make_inputs(row)
        _REF[row["name"]] = RR.recall_ref(z, t, ignore_index(row))
    return _REF[row["name"]]


# ------------------------------------------------------------------------------------------------ helpers
def _losses():
    from crop2seg_amd import engine as E
    from crop2seg_amd.learning import losses
    return E, losses


def dev():
    return torch.device("cuda")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def observe(name, ratio):
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), ratio)
    print(f"  recall   {name:10s} ratio {ratio:.3f}")


def check(name, got, ref, A, frob, max_rel=None):
    got = got.detach().double().cpu().reshape(ref[name].shape)
    if max_rel is not None:
        err, top = float((got - ref[name]).abs().max()), float(ref[name].abs().max())
        print(f"  recall   {name:10s} max err {err:.3e} of max {top:.3e}")
        assert err <= max_rel * top, f"recall {name}: max error {err:.3e} > {max_rel:g} * {top:.3e}"
    observe(name, assert_within(f"recall {name}", got, ref[name], A[name], R.C_BOUND, frob))


def check_integers(losses, ws, row, ref, weights, counts):
    assert np.array_equal(counts.cpu().numpy(), ref["counts"]), "gt / fn counts"
    assert np.array_equal(weights.cpu().numpy().view(np.int32), ref["weights"].view(np.int32)), "class weights, bit for bit"
    assert int(float(losses.recall_bad_targets(ws, row["B"], row["H"] * row["W"]))) == ref["bad"], "bad-label count"


def run_row(row):
    E, losses = _losses()
    z, t = make_inputs(row)
    ref, A = reference(row)
    n = pixels(row)
    ws = E.Workspace(dev())
    zd, td = z.cuda(), t.cuda()
    loss, gl, weights, counts = losses.recall_ce(zd, td, ignore_index(row), True, ws)
    check_integers(losses, ws, row, ref, weights, counts)
    buf = ws.bufs["recall"]
    size = losses.lib().c2s_recall_ce_workspace_floats(row["B"], row["H"] * row["W"])
    check("loss", loss, ref, A, R.SCALAR_REL)
    check("glogits", gl, ref, A, 1e-5, R.GRAD_MAX_REL)
    check("nll", buf[:n].clone(), ref, A, 1e-5)
    check("tot", buf[size - 2:size - 1].clone(), ref, A, R.SCALAR_REL)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gl).all())
    loss2, gl2, weights2, counts2 = losses.recall_ce(zd, td, ignore_index(row), True, ws)
    assert same_bits(loss, loss2) and same_bits(gl, gl2), "two consecutive calls differ"
    assert same_bits(weights, weights2) and torch.equal(counts, counts2), "the counters were not zeroed between two calls"
    loss3, none, _, _ = losses.recall_ce(zd, td, ignore_index(row), False, ws)
    assert none is None and same_bits(loss, loss3), "the forward-only call gives another loss"
    if row.get("all_ignored"):
        assert bool((bits(loss) == 0).all()) and bool((bits(gl) == 0).all()), "nothing valid: loss and gradient are exactly 0"
    RAN.add(row["name"])


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("row", ROWS, ids=ids(ROWS))
def test_recall_ce(row, monkeypatch):
    if pixels(row) % 256 == 0:
        run_row(row)
        return
    import test_redzone_gpu as TRZ
    TRZ.in_arena(TRZ.Case(f"recall/{row['name']}", lambda mp: run_row(row), mib=16), monkeypatch)


def by_name(name):
    return next(r for r in ROWS if r["name"] == name)


def test_call_after_another_shape_on_the_same_workspace():
    E, losses = _losses()
    ws = E.Workspace(dev())
    for name in ("recall_hw257_k15", "recall_hw5_k2", "recall_hw63_k20"):      # larger, smaller, larger again
        row = by_name(name)
        z, t = make_inputs(row)
        ref, A = reference(row)
        loss, gl, weights, counts = losses.recall_ce(z.cuda(), t.cuda(), ignore_index(row), True, ws)
        check_integers(losses, ws, row, ref, weights, counts)
        fresh = losses.recall_ce(z.cuda(), t.cuda(), ignore_index(row), True, E.Workspace(dev()))
        assert same_bits(loss, fresh[0]) and same_bits(gl, fresh[1]), f"{name}: a used workspace gives other bits"
        check("loss", loss, ref, A, R.SCALAR_REL)


def test_accumulate_loss_adds():
    E, losses = _losses()
    row = by_name("recall_hw257_k15")
    z, t = make_inputs(row)
    ws = E.Workspace(dev())
    plain, _, _, _ = losses.recall_ce(z.cuda(), t.cuda(), ignore_index(row), False, ws)
    prior = torch.tensor([0.25], dtype=torch.float32)
    acc = prior.cuda()
    out, gl, _, _ = losses.recall_ce(z.cuda(), t.cuda(), ignore_index(row), True, ws, acc)
    assert out.data_ptr() == acc.data_ptr()
    assert same_bits(out.cpu(), prior + plain.cpu()), "loss_out: the value is not prior + loss"
    ref, A = RR.recall_ref(z, t, ignore_index(row), prior=prior)
    check("loss", out, ref, A, R.SCALAR_REL)
    check("glogits", gl, ref, A, 1e-5, R.GRAD_MAX_REL)


def test_more_than_32_classes_raise():
    E, losses = _losses()
    z = torch.zeros(1, 33, 2, 2, device=dev())
    t = torch.zeros(1, 2, 2, dtype=torch.int64, device=dev())
    with pytest.raises(ValueError, match="32"):
        losses.recall_ce(z, t)
    with pytest.raises(ValueError, match="32"):
        losses.RecallCrossEntropy(n_classes=33)
    L = losses.lib()
    ws = torch.empty(L.c2s_recall_ce_workspace_floats(1, 4), device=dev())
    loss = torch.empty(1, device=dev())
    rc = L.c2s_recall_ce(z.data_ptr(), t.data_ptr(), loss.data_ptr(), None, None, None, 1, 33, 4, 255, 0, ws.data_ptr(),
                         ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"32" in L.c2s_last_error()


def test_class_is_the_function():
    E, losses = _losses()
    row = by_name("recall_hw257_k15")           # bad labels, ignore_index -100
    assert row["bad"]
    z, t = make_inputs(row)
    ref, _ = reference(row)
    zd, td = z.cuda(), t.cuda()
    loss, gl, weights, counts = losses.recall_ce(zd, td, ignore_index(row), True)
    crit = losses.RecallCrossEntropy(n_classes=15, ignore_index=ignore_index(row))
    assert crit.grad() is None and crit.bad_target_count() == 0
    value = crit(zd, td, want_grad=True)
    assert value.dim() == 0 and same_bits(value.reshape(1), loss) and same_bits(crit.grad(), gl)
    assert same_bits(crit.class_weights(), weights) and torch.equal(crit.counts(), counts)
    assert crit.bad_target_count() == ref["bad"] > 0
    with pytest.raises(ValueError, match="outside"):
        crit.check_targets()
    assert same_bits(crit.forward(zd, td).reshape(1), loss) and crit.grad() is None
    with pytest.raises(ValueError, match="classes"):
        losses.RecallCrossEntropy(n_classes=19)(zd, td)
    clean = losses.RecallCrossEntropy(n_classes=15, ignore_index=255)
    clean(zd, td.clamp(0, 14))
    clean.check_targets()


# ------------------------------------------------------------------------------------------------ TrainStep(criterion=...)
def fresh(boundary=False, **kw):
    """The smallest U-TAE the constructor takes, in the seeded "tame" state, and its TrainStep."""
    import crop2seg_amd as C2S
    from crop2seg_amd.learning.utils import TrainStep
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=[32, 15], add_boundary_loss=boundary)
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    net = net.cuda().train()
    return net, TrainStep(net, num_classes=15, **kw)


_BATCH = {}


def batch():
    """x [2,3,10,32,32], dates, and three label maps: y (clean), y1 / y2 (some pixels 255 = ignored, two labels outside [0, 15))."""
    from oracle import seeded
    if not _BATCH:
        x, dates, y = seeded.make_inputs(2, 3, 10, 32, 32, 91, [3, 2])
        ys = [y]
        for seed in (92, 93):
            g = torch.Generator().manual_seed(seed)
            yy = torch.randint(0, 15, y.shape, generator=g)
            yy[torch.rand(y.shape, generator=g) < 0.25] = 255
            yy[0, 0, 0], yy[1, 31, 31] = 77, -3
            ys.append(yy)
        _BATCH["dev"] = (x.cuda(), dates.cuda(), [v.cuda() for v in ys])
    return _BATCH["dev"]


def drop_state():
    from crop2seg_amd.backbones import functional as Fn
    return Fn.DropoutState(attn_seed=11, mlp_seed=12)


def test_trainstep_criterion_none_is_the_step_without_the_argument():
    x, d, (y, _, _) = batch()
    _, step_a = fresh()
    _, step_b = fresh(criterion=None)
    for _ in range(2):
        la, za = step_a(x, d, y, dropout_state=drop_state())
        lb, zb = step_b(x, d, y, dropout_state=drop_state())
        assert same_bits(la, lb) and same_bits(za, zb)
    assert same_bits(step_a.flat_grad, step_b.flat_grad) and same_bits(step_a.flat_param, step_b.flat_param)


class Stub:
    """A criterion that hands back a stored (loss, gradient) pair: the plumbing without new numerics."""

    def __init__(self, loss, grad):
        self.loss, self._grad, self.calls = loss, grad, 0

    def __call__(self, logits, y, want_grad=False):
        assert want_grad and logits.shape == self._grad.shape
        self.calls += 1
        return self.loss.clone()[0]

    def grad(self):
        return self._grad.clone()


def test_trainstep_recall_criterion_eager():
    E, losses = _losses()
    x, d, (_, y1, _) = batch()
    crit = losses.RecallCrossEntropy(n_classes=15, ignore_index=255)
    _, step = fresh(criterion=crit)
    loss, logits = step(x, d, y1, dropout_state=drop_state(), apply_update=False)
    assert loss.shape == (1,)
    want, grad, weights, _ = losses.recall_ce(logits, y1, 255, True)
    assert same_bits(loss, want), "the step's loss is not recall_ce of its logits"
    assert same_bits(crit.class_weights(), weights)
    assert step.bad_targets() == crit.bad_target_count() == 2
    stub = Stub(want, grad)
    _, twin = fresh(criterion=stub)
    loss2, logits2 = twin(x, d, y1, dropout_state=drop_state(), apply_update=False)
    assert stub.calls == 1 and same_bits(logits, logits2) and same_bits(loss, loss2)
    assert same_bits(step.flat_grad, twin.flat_grad), "the criterion's gradient did not reach the tape as it is"
    assert bool(torch.isfinite(step.flat_grad).all()) and float(step.flat_grad.abs().max()) > 0
    assert twin.bad_targets() == 0


def test_trainstep_recall_criterion_with_boundary_head():
    E, losses = _losses()
    x, d, (_, y1, _) = batch()
    _, step = fresh(boundary=True, criterion=losses.RecallCrossEntropy(n_classes=15, ignore_index=255))
    loss, logits = step(x, d, y1, dropout_state=drop_state(), apply_update=False)
    want, _, _, _ = losses.recall_ce(logits, y1, 255)
    main = want.clone()
    losses.focal_ce(step.last_boundary, losses.boundary_target(y1), step.boundary_gamma, loss_out=want)
    assert same_bits(loss, want) and not same_bits(loss, main), "loss != recall_ce followed by focal_ce(loss_out=...)"


def test_trainstep_recall_criterion_captured():
    E, losses = _losses()
    x, d, (y, y1, y2) = batch()
    crit = losses.RecallCrossEntropy(n_classes=15, ignore_index=255)
    _, step = fresh(criterion=crit)
    step.capture(x, d, y)
    seen = []
    for yy in (y1, y2):
        loss, logits = step.replay(x, d, yy)
        loss, logits = loss.clone(), logits.clone()
        want, _, weights, _ = losses.recall_ce(logits, yy, 255)
        assert same_bits(loss, want), "a replay's loss is not recall_ce of that replay's logits"
        assert same_bits(crit.class_weights(), weights), "stale weights in the replayed graph"
        seen.append(loss)
    assert not same_bits(seen[0], seen[1])
    assert step.bad_targets() == 2


def test_trainstep_focal_and_smooth_criteria():
    E, losses = _losses()
    from crop2seg_amd.learning.utils import TrainStep
    x, d, (y, y1, _) = batch()
    for make, labels in ((lambda: losses.FocalCELoss(gamma=2.0, ignore_index=255), y1),
                         (lambda: losses.SmoothCrossEntropy2D(label_smoothing=0.1), y)):
        _, step = fresh(criterion=make())
        loss, logits = step(x, d, labels, dropout_state=drop_state(), apply_update=False)
        again = make()(logits, labels)
        assert same_bits(loss, again.reshape(1)), "the step's loss is not the criterion on its logits"
        assert bool(torch.isfinite(step.flat_grad).all()) and float(step.flat_grad.abs().max()) > 0
    net, _ = fresh()
    with pytest.raises(ValueError, match="none"):
        TrainStep(net, num_classes=15, criterion=losses.SmoothCrossEntropy2D(reduction="none"))
    with pytest.raises(TypeError):
        TrainStep(net, num_classes=15, criterion=lambda a, b, want_grad=False: None)


# ------------------------------------------------------------------------------------------------ closing
def table_coverage():
    """What the row table reaches, from the table alone (also asserted on the CPU by test_recall_reference.py)."""
    main = [r for r in ROWS if r["name"].startswith("recall_hw")]
    return {
        "grid": [r["name"] for r in ROWS if pixels(r) > max(RECALL_COUNT_CAP, RECALL_LOSS_CAP, RECALL_BWD_CAP) and r["K"] == 2],
        "K": sorted({r["K"] for r in main}),
        "HW": sorted({r["W"] for r in main}),
        "kinds": sorted({r["logits"] for r in main}),
        "ignore": sorted({(str(r["ignore"]), bool(r["bad"])) for r in main}),
        "arena": [r["name"] for r in ROWS if pixels(r) % 256 != 0],
        "named": sorted(r["name"] for r in ROWS if not r["name"].startswith("recall_hw")),
    }


def assert_table_coverage():
    c = table_coverage()
    assert c["grid"] == ["recall_grid"]
    assert c["K"] == [1, 2, 15, 20, 32] and c["HW"] == [1, 5, 63, 257] and c["kinds"] == sorted(LOGIT_KINDS)
    assert c["ignore"] == sorted((str(i), b) for i in IGNORES for b in (False, True))
    assert "recall_hw257_k15" in c["arena"] and "recall_grid" in c["arena"]
    assert c["named"] == sorted(["perfect", "all_wrong", "one_class", "all_ignored", "class1_perfect_with_ignored", "ties_k2",
                                 "aligned", "recall_grid"])


def test_rows_reach_every_path():
    """Every row of the table ran (and passed), and the table holds the grid row, every K edge and every ignore_index."""
    assert_table_coverage()
    names = {r["name"] for r in ROWS}
    assert names <= RAN, f"rows that did not run or did not pass: {sorted(names - RAN)}"
    print("  worst ratio |err| / (u A)  recall    " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(OBSERVED.items())))
