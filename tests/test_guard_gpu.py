"""The guarded optimiser step on the GPU (csrc/guard.hip; TrainStep(max_grad_norm=..., skip_nonfinite=...)): the four entry
points one by one against numpy float64 / tests/guard_ref.py, then TrainStep on U-TAE -- defaults untouched, a guard that never
fires bit-identical to the unguarded step (eager and replayed), clipping against guard_ref, a NaN batch and a poisoned
normalisation sync area skipped without a trace, a parameter frozen across the skipped step -- and the guarded step through RCCL.

Bars.  Sum of squares: n * 2^-53 relative (a sum of n non-negative float64 terms in any order).  Clip coefficient: 2 float32 ulps
(one rounding to float32 plus the float64 noise of sqrt and the division).  Adam: tail_ref.ADAM_FROB / adam_upd_frob and the
per-element bound C_BOUND * u * A of tests/tail_ref.py, the reference fed the float32 scale * coef read back from the status
block."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import guard_ref as G
import tail_ref as R
from tail_ref import assert_within

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 2048                  # floats one workgroup pass covers (GD_CHUNK of csrc/guard.hip)
NAN = float("nan")


def _E():
    from crop2seg_amd import engine as E
    return E


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


class Table:
    """A slot table on the device with everything the entry points take."""

    def __init__(self, slots, flags, total, steps=None):
        E = _E()
        self.slots, self.flags, self.total = slots, flags, total
        self.slots_dev = torch.tensor(slots, device="cuda", dtype=torch.int64)
        self.mask_dev = torch.tensor([1 if f else 0 for f in flags], device="cuda", dtype=torch.int32)
        self.steps_dev = torch.tensor(steps if steps is not None else [0] * len(slots), device="cuda", dtype=torch.int32)
        self.skip_dev = torch.zeros(1, device="cuda", dtype=torch.int32)
        self.status = E.guard_status("cuda")
        self.views = E.guard_views(self.status)
        self.ws = E.Workspace(torch.device("cuda"))

    def inside(self):
        """bool [total]: elements of trainable slots."""
        m = torch.zeros(self.total, dtype=torch.bool)
        for (o, n), f in zip(self.slots, self.flags):
            if f:
                m[o:o + n] = True
        return m


# lengths 1, 3, 255, 257 and one slot of 2048 * k + 3; the slot of 257 is frozen between two trainable ones; the slot of 2051
# starts at 2044 and ends at 4095, so the chunk that starts at 4096 starts inside padding and the workgroups of chunks 0 and 1
# straddle slot boundaries; behind the last slot there is padding up to `total`
SMALL = dict(slots=[(0, 1), (4, 3), (8, 255), (264, 257), (524, 5), (2044, CHUNK + 3), (4100, 300)],
             flags=[True, True, True, False, True, True, True], total=4403)
# more than 256 chunks: every workgroup of the sum reduces two chunks, the last one a short range
LARGE = dict(slots=[(0, 7), (8, CHUNK * 300 + 3), (CHUNK * 300 + 12, 129)], flags=[True, True, True], total=CHUNK * 300 + 150)


def fill(layout, seed, scale=1.0):
    """float32 [total]: random inside the trainable slots, NaN in the frozen slots and in the padding (neither may be read)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((layout["total"],), NAN)
    for (o, n), f in zip(layout["slots"], layout["flags"]):
        if f:
            g[o:o + n] = torch.randn(n, generator=gen) * scale
    return g


# ------------------------------------------------------------------------------------------------ 1. c2s_grad_sumsq
@pytest.mark.parametrize("layout,kind", [(SMALL, "normal"), (SMALL, "1e30"), (SMALL, "inf"), (SMALL, "nan"), (LARGE, "normal")],
                         ids=["small", "small_1e30", "small_inf", "small_nan", "large"])
def test_grad_sumsq(layout, kind):
    E = _E()
    t = Table(**layout)
    g = fill(layout, 3)
    if kind == "1e30":                           # squares overflow float32: the sum must stay finite and exact to the bar
        g = torch.where(torch.isnan(g), g, torch.sign(g) * 1e30 + (g == 0) * 1e30)
    elif kind == "inf":
        g[2044 + 77] = float("inf")
    elif kind == "nan":
        g[4100 + 299] = NAN                      # the last element of the last trainable slot
    gd = g.cuda()
    E.grad_sumsq(gd, t.slots_dev, t.mask_dev, t.ws, t.status)
    got = float(t.views["sumsq"])
    raw = bits(t.status).clone()
    ref, n = G.sumsq_ref(g.numpy(), layout["slots"], layout["flags"])
    print(f"  sumsq {kind}: got {got!r} ref {ref!r} over {n} elements")
    if kind == "inf":
        assert got == float("inf") and ref == float("inf")
    elif kind == "nan":
        assert got != got and ref != ref
    else:
        assert np.isfinite(got) and abs(got - ref) <= n * 2.0 ** -53 * ref
    # flagged or not: the decision launch on this sum
    E.step_decide(t.status, None, 1.0, True, t.mask_dev, t.steps_dev, t.skip_dev)
    assert int(t.views["ok"]) == (0 if kind in ("inf", "nan") else 1)
    # a second run gives the same bits
    t.status.zero_()
    E.grad_sumsq(gd, t.slots_dev, t.mask_dev, t.ws, t.status)
    assert bool((bits(t.status)[:2] == raw[:2]).all())


# ------------------------------------------------------------------------------------------------ 2. c2s_step_decide
DECIDE_ROWS = [  # sumsq, max_grad_norm, grad_scale, skip_nonfinite
    (9.0, 1.0, 1.0, True), (9.0, 5.0, 1.0, True), (1234.5678, 0.3, 0.5, True), (2.0e-13, 1e-6, 1.0, False),
    (1e60, 7.0, 0.125, True), (0.0, 1.0, 1.0, True), (7.0, None, 0.25, True), (float("inf"), 1.0, 1.0, True),
    (NAN, 1.0, 1.0, True), (float("inf"), 1.0, 1.0, False), (NAN, None, 1.0, False), (3.0, 1e30, 1.0, True)]


@pytest.mark.parametrize("ss,max_norm,gs,skip", DECIDE_ROWS, ids=[f"row{i}" for i in range(len(DECIDE_ROWS))])
def test_step_decide(ss, max_norm, gs, skip):
    E = _E()
    t = Table(slots=[(0, 4), (4, 4), (8, 4), (12, 4)], flags=[True, False, True, True], total=16, steps=[5, 9, 0, 70000])
    t.status[0] = ss
    E.step_decide(t.status, max_norm, gs, skip, t.mask_dev, t.steps_dev, t.skip_dev)
    ok, norm, coef, scale = G.decide_ref(ss, max_norm, gs, skip)
    got = {k: v.item() for k, v in t.views.items()}
    print(f"  decide: got {got}  ref ok {ok} norm {norm!r} coef {coef!r} scale {scale!r}")
    assert got["ok"] == int(ok)
    for name, want in (("coef", coef), ("scale", scale), ("norm", norm)):
        w32 = np.float32(want)
        if np.isfinite(w32):
            assert abs(np.float64(np.float32(got[name])) - np.float64(w32)) <= 2 * np.float64(np.spacing(np.abs(w32))), name
        else:
            assert (got[name] != got[name]) if want != want else got[name] == want, name
    if max_norm == 1e30 or max_norm is None:
        assert got["coef"] == 1.0 and got["scale"] == float(np.float32(gs))          # exactly: the bit-identity of a guard that
    want_steps = [6, 9, 1, 70001] if ok else [5, 9, 0, 70000]                        # never fires rests on it
    assert t.steps_dev.tolist() == want_steps and int(t.skip_dev) == (0 if ok else 1)
    E.step_decide(t.status, max_norm, gs, skip, t.mask_dev, t.steps_dev, t.skip_dev)
    assert t.steps_dev.tolist() == ([7, 9, 2, 70002] if ok else want_steps) and int(t.skip_dev) == (0 if ok else 2)


# ------------------------------------------------------------------------------------------------ 3. c2s_adam_slots
def adam_state(layout, seed):
    """p, g, m, v float32 [total] as tail_ref.make_adam_inputs draws them; g NaN outside the trainable slots."""
    gen = torch.Generator().manual_seed(seed)
    tot = layout["total"]
    p = torch.randn(tot, generator=gen) * 1e-2
    m = torch.randn(tot, generator=gen) * 0.1
    v = torch.rand(tot, generator=gen) * 0.01
    return p, fill(layout, seed + 1), m, v


def check_slots(what, ref, got_p, got_m, got_v, p0, slots):
    """Every slot that stepped against its adam_ref, at the bars of tests/test_tail_reference_gpu.py::test_adam."""
    worst = 0.0
    for i, (o, A) in ref["per_slot"].items():
        off, n = slots[i]
        s = slice(off, off + n)
        for name, got in (("m", got_m), ("v", got_v), ("p", got_p)):
            worst = max(worst, assert_within(f"{what} slot {i} {name}", got[s].cpu(), o[name], A[name], R.C_BOUND, R.ADAM_FROB))
        upd = got_p[s].double().cpu() - p0[s].double().cpu()
        worst = max(worst, assert_within(f"{what} slot {i} upd", upd, o["upd"], A["upd"], R.C_BOUND, R.adam_upd_frob(o, A)))
    return worst


@pytest.mark.parametrize("max_norm,gs", [(None, 1.0), (0.37, 0.125)], ids=["coef1", "clipped"])
def test_adam_slots_against_adam_ref(max_norm, gs):
    E = _E()
    steps = [0, 1, 9, 4, 999, 99999, 1]
    t = Table(**SMALL, steps=steps)
    p, g, m, v = adam_state(SMALL, 21)
    pd, gd, md, vd = p.cuda(), g.cuda(), m.cuda(), v.cuda()
    E.grad_sumsq(gd, t.slots_dev, t.mask_dev, t.ws, t.status)
    E.step_decide(t.status, max_norm, gs, True, t.mask_dev, t.steps_dev, t.skip_dev)
    E.adam_slots(pd, gd, md, vd, t.slots_dev, t.mask_dev, t.steps_dev, t.status)
    scale32 = float(t.views["scale"])
    ref = G.guard_ref(p, g, m, v, steps, SMALL["slots"], SMALL["flags"], max_grad_norm=max_norm, skip_nonfinite=True,
                      grad_scale=gs, scale32=scale32)
    assert ref["ok"] and int(t.views["ok"]) == 1 and t.steps_dev.tolist() == ref["steps"]
    assert (ref["coef"] < 1.0) == (max_norm is not None)
    assert abs(scale32 - ref["scale"]) <= 2 * float(np.spacing(np.float32(ref["scale"])))
    worst = check_slots("adam_slots", ref, pd, md, vd, p, SMALL["slots"])
    print(f"  adam_slots: worst ratio {worst:.3f}")
    out = ~t.inside()                                             # the frozen slot and the padding: not written
    assert same_bits(pd.cpu()[out], p[out]) and same_bits(md.cpu()[out], m[out]) and same_bits(vd.cpu()[out], v[out])
    assert same_bits(gd.cpu(), g)


def test_adam_slots_skipped_step_writes_nothing():
    E = _E()
    steps = [3, 1, 9, 4, 999, 99999, 1]
    t = Table(**SMALL, steps=steps)
    p, g, m, v = adam_state(SMALL, 22)
    g[8 + 100] = float("inf")
    pd, gd, md, vd = p.cuda(), g.cuda(), m.cuda(), v.cuda()
    E.grad_sumsq(gd, t.slots_dev, t.mask_dev, t.ws, t.status)
    E.step_decide(t.status, 1.0, 1.0, True, t.mask_dev, t.steps_dev, t.skip_dev)
    E.adam_slots(pd, gd, md, vd, t.slots_dev, t.mask_dev, t.steps_dev, t.status)
    saved = torch.arange(40, device="cuda", dtype=torch.float32)
    dst = torch.full((40,), NAN, device="cuda")
    E.restore_if_skipped(dst, saved, t.status)
    assert int(t.views["ok"]) == 0 and int(t.skip_dev) == 1 and t.steps_dev.tolist() == steps
    assert same_bits(pd.cpu(), p) and same_bits(md.cpu(), m) and same_bits(vd.cpu(), v)
    assert torch.equal(dst, saved)                                # skipped: the buffers are put back ...
    t.status[0] = 4.0
    E.step_decide(t.status, 1.0, 1.0, True, t.mask_dev, t.steps_dev, t.skip_dev)
    dst.fill_(7.0)
    E.restore_if_skipped(dst, saved, t.status)
    assert int(t.views["ok"]) == 1 and bool((dst == 7.0).all())   # ... applied: they stay


@pytest.mark.parametrize("step,gs", [(1, 1.0), (1000, 0.5)])
def test_adam_slots_equals_adam_flat(step, gs):
    """coef = 1 and equal step counts: bit-identical to c2s_adam_flat on the same data (slots that tile the buffer, and a
    buffer long enough for adam_flat's grid-stride pass)."""
    E = _E()
    sizes = [4, 260, 2048 * 257 + 8, 12]
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += s
    layout = dict(slots=list(zip(offs, sizes)), flags=[True] * len(sizes), total=o)
    t = Table(**layout, steps=[step - 1] * len(sizes))
    p, g, m, v = adam_state(layout, 23)
    a = [x.cuda() for x in (p, g, m, v)]
    b = [x.cuda() for x in (p, g, m, v)]
    E.grad_sumsq(a[1], t.slots_dev, t.mask_dev, t.ws, t.status)
    E.step_decide(t.status, None, gs, True, t.mask_dev, t.steps_dev, t.skip_dev)
    E.adam_slots(*a, t.slots_dev, t.mask_dev, t.steps_dev, t.status)
    E.adam_flat(*b, step, grad_scale=gs)
    for x, y, name in zip(a, b, "pgmv"):
        assert same_bits(x, y), name
    assert not same_bits(a[0].cpu(), p)


# ------------------------------------------------------------------------------------------------ 4. TrainStep on U-TAE
def fresh(**kw):
    """U-TAE in the seeded "tame" state of the recovery test (tests/test_models_gpu.py), dropout off, and its TrainStep."""
    import crop2seg_amd as C2S
    from crop2seg_amd.learning.utils import TrainStep
    from oracle import seeded
    net = C2S.UTAE(input_dim=10, out_conv=[32, 15])
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = seeded.make_state(ks, 3, "tame")
    net.load_state_dict(sd)
    net = net.cuda().train()
    net.spec.attn_dropout = 0.0
    net.spec.mlp_dropout = 0.0
    return net, TrainStep(net, num_classes=15, **kw), sd


_BATCH = {}


def batch():
    from oracle import seeded
    if not _BATCH:
        x, dates, y = seeded.make_inputs(2, 4, 10, 32, 32, 91, [4, 3])
        _BATCH["host"] = (x, dates, y)
        _BATCH["dev"] = (x.cuda(), dates.cuda(), y.cuda())
        xn = x.clone()
        xn[1, 2, 3, 17, 5] = NAN                                   # one NaN pixel
        _BATCH["nan"] = (xn.cuda(), dates.cuda(), y.cuda())
    return _BATCH


def state_of(step):
    """Host copies of everything a skipped step must leave alone."""
    s = {"p": step.flat_param, "m": step.exp_avg, "v": step.exp_avg_sq}
    if getattr(step, "flat_buf", None) is not None:
        s["buf"] = step.flat_buf
    if step.guarded:
        s["steps"] = step.slot_steps_dev
    return {k: t.detach().cpu().clone() for k, t in s.items()}


def assert_same_state(a, b, keys=None):
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and bool((a[k].view(torch.int32) == b[k].view(torch.int32)).all()), k


def assert_finite(step, net):
    for t in (step.flat_param, step.exp_avg, step.exp_avg_sq):
        assert bool(torch.isfinite(t).all())
    for k, b in net.named_buffers():
        if b.is_floating_point():
            assert bool(torch.isfinite(b).all()), k


def test_trainstep_defaults_launch_nothing_new(monkeypatch):
    """(a) Both options at their defaults: bit-identical to a twin built without the arguments; no new entry point runs."""
    E = _E()
    x, d, y = batch()["dev"]
    net_a, step_a, _ = fresh()
    for _ in range(3):
        step_a(x, d, y)

    def forbidden(*a, **k):
        raise AssertionError("a guard entry point ran in an unguarded step")

    for name in ("grad_sumsq", "step_decide", "adam_slots", "restore_if_skipped"):
        monkeypatch.setattr(E, name, forbidden)
    net_b, step_b, _ = fresh(max_grad_norm=None, skip_nonfinite=False)
    assert not step_b.guarded
    for _ in range(3):
        step_b(x, d, y)
    assert_same_state(state_of(step_a), state_of(step_b))
    for (k, a), (_, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(a, b), k
    with pytest.raises(RuntimeError, match="no guarded step"):
        step_b.skipped_steps()


def test_trainstep_guard_that_never_fires_is_bit_identical_eager_and_replayed():
    """(b) max_grad_norm=1e30, skip_nonfinite=True: three eager steps, then three replays, against the unguarded twin."""
    x, d, y = batch()["dev"]
    net_u, step_u, _ = fresh()
    net_g, step_g, _ = fresh(max_grad_norm=1e30, skip_nonfinite=True)
    for _ in range(3):
        lu, _ = step_u(x, d, y)
        lg, _ = step_g(x, d, y)
    assert float(lu) == float(lg)
    assert_same_state(state_of(step_u), state_of(step_g), ("p", "m", "v"))
    step_g.capture(x, d, y)
    for _ in range(3):
        lu, _ = step_u(x, d, y)
        lg, _ = step_g.replay()
    torch.cuda.synchronize()
    assert float(lu) == float(lg)
    assert_same_state(state_of(step_u), state_of(step_g), ("p", "m", "v"))
    for (k, a), (_, b) in zip(net_u.state_dict().items(), net_g.state_dict().items()):
        assert torch.equal(a, b), k
    assert step_g.skipped_steps() == 0 and float(step_g.last_clip_coef) == 1.0
    step_g.sync_steps()
    assert step_g.param_steps == step_u.param_steps == [6] * len(step_u.param_steps) and step_g.step_count == 6


def slots_of(step):
    from crop2seg_amd.learning.utils import slot_table
    return slot_table(step.offsets, step.total, [True] * len(step.offsets))[0]


def test_trainstep_clips_like_guard_ref():
    """(c) max_grad_norm = half the norm of the first step's gradient: every step against guard_ref fed flat_grad read back."""
    x, d, y = batch()["dev"]
    _, probe, _ = fresh()
    probe(x, d, y, apply_update=False)
    norm0 = float(probe.flat_grad.double().norm())
    max_norm = 0.5 * norm0
    net, step, _ = fresh(max_grad_norm=max_norm)
    slots, flags = slots_of(step), step.trainable_flags()
    steps = [0] * len(slots)
    for it in range(3):
        before = state_of(step)
        step(x, d, y)
        g = step.flat_grad.cpu()
        scale32 = float(E_views(step)["scale"])
        ref = G.guard_ref(before["p"], g, before["m"], before["v"], steps, slots, flags, max_grad_norm=max_norm, scale32=scale32)
        norm64 = float(np.sqrt(G.sumsq_ref(g.numpy(), slots, flags)[0]))
        got_norm, got_coef = float(step.last_grad_norm), float(step.last_clip_coef)
        print(f"  step {it}: norm {got_norm!r} (float64 {norm64!r}) coef {got_coef!r} (ref {ref['coef']!r}) max_norm {max_norm!r}")
        assert ref["coef"] < 1.0, "clipping is not active"
        assert abs(got_norm - float(np.float32(norm64))) <= 2 * float(np.spacing(np.float32(norm64)))
        assert abs(got_coef - float(np.float32(ref["coef"]))) <= 2 * float(np.spacing(np.float32(ref["coef"])))
        worst = check_slots(f"step {it}", ref, step.flat_param, step.exp_avg, step.exp_avg_sq, before["p"], slots)
        print(f"  step {it}: worst ratio {worst:.3f}")
        steps = ref["steps"]
        assert step.slot_steps_dev.tolist() == steps
    assert_finite(step, net)


def E_views(step):
    return _E().guard_views(step._status)


def test_trainstep_skips_a_nan_batch_eager_and_replayed():
    """(d) One NaN pixel in x, apply_update=True: nothing changes, the skip is counted, the next clean step trains."""
    x, d, y = batch()["dev"]
    xn, _, _ = batch()["nan"]
    net, step, _ = fresh(skip_nonfinite=True)
    step(x, d, y)
    for mode in ("eager", "replay"):
        if mode == "replay":
            step.capture(x, d, y)
        run = (lambda *a: step(*a)) if mode == "eager" else (lambda *a: step.replay(*a))
        before = state_of(step)
        nbt = {k: int(b) for k, b in net.named_buffers() if k.endswith("num_batches_tracked")}
        skipped0 = step.skipped_steps()
        loss, _ = run(xn, d, y)                                   # (the ReLU after the first normalisation turns the NaN
        print(f"  {mode}: loss of the NaN batch {float(loss)!r}")     # activations into zeros: the loss may well be finite)
        assert_same_state(before, state_of(step))
        assert step.skipped_steps() == skipped0 + 1
        assert all(int(b) >= nbt[k] for k, b in net.named_buffers() if k in nbt)
        assert_finite(step, net)
        loss, _ = run(x, d, y)
        after = state_of(step)
        assert float(loss) == float(loss) and not torch.equal(after["p"], before["p"])
        assert (after["steps"] == before["steps"] + 1).all()
        assert_finite(step, net)
    assert step.skipped_steps() == 2
    assert step.param_steps == [5] * len(step.param_steps)            # the host counted the skipped steps as taken ...
    step.sync_steps()
    assert step.param_steps == [3] * len(step.param_steps) and step.step_count == 3       # ... until sync_steps()


def test_trainstep_survives_a_failed_normalisation_wait(monkeypatch):
    """(e) The sync area's error word pre-set, skip_nonfinite=True, apply_update=True: the health check still raises, the
    optimiser state and the BatchNorm statistics are finite and unchanged, the next step (two-pass kernels) equals the oracle's."""
    from oracle import crop2seg_oracle as O
    from crop2seg_amd import engine as E
    from crop2seg_amd.learning.metrics import StepMeters
    monkeypatch.setattr(E, "ONEPASS_NORM", True)
    x, dates, y = batch()["host"]
    xd, dd, yd = batch()["dev"]
    net, step, sd = fresh(skip_nonfinite=True)
    meters = StepMeters(15, ignore_index=-1).watch(step)
    loss, logits = step(xd, dd, yd, apply_update=False)
    assert step.bad_targets() == 0
    ref_logits, ref_loss, grads, _ = O.loss_and_grads(sd, x, dates, y, O.BackboneConfig(), True)
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    # the step above was not applied but its forward pass moved the running statistics: the state a skipped step must keep
    before = state_of(step)
    rm = {k: b.detach().cpu().clone() for k, b in net.named_buffers() if k.endswith(("running_mean", "running_var"))}
    assert rm
    step.ws.bufs["sync"][:16].view(torch.int32)[3] = 1       # a wait gave up
    loss, logits = step(xd, dd, yd, apply_update=True)
    meters.update(logits, yd, loss)
    with pytest.raises(RuntimeError, match="one-pass normalisation wait gave up"):
        meters.loss_mean()
    assert E.ONEPASS_NORM is False
    print(f"  poisoned step: loss {float(loss)!r} skipped {step.skipped_steps()}")
    assert_finite(step, net)
    assert_same_state(before, state_of(step))
    for k, b in net.named_buffers():
        if k in rm:
            assert torch.equal(b.cpu(), rm[k]), k
    loss, logits = step(xd, dd, yd, apply_update=True)       # two-pass kernels: same numbers as the oracle again
    assert step.bad_targets() == 0
    assert abs(float(loss) - float(ref_loss)) < 1e-3 * abs(float(ref_loss))
    assert float((logits.cpu() - ref_logits).abs().max()) < 1e-3 * float(ref_logits.abs().max())
    n = "in_conv.conv.conv.0.weight"
    assert float((step.grads[n].cpu() - grads[n]).norm() / grads[n].norm()) < 1e-3
    assert_finite(step, net)
    assert not torch.equal(step.flat_param.cpu(), before["p"])


def test_trainstep_parameter_frozen_across_the_skipped_step():
    """(f) clean; frozen + clean; frozen + NaN batch (skipped); unfrozen + clean: the device step counts and every update
    against guard_ref -- the skip counts against nobody, the frozen steps only against the frozen parameter."""
    x, d, y = batch()["dev"]
    xn, _, _ = batch()["nan"]
    net, step, _ = fresh(skip_nonfinite=True, max_grad_norm=1e30)
    name = "in_conv.conv.conv.0.weight"
    k = step.names.index(name)
    param = dict(net.named_parameters())[name]
    slots = slots_of(step)
    steps = [0] * len(slots)
    for it, (frozen, bad) in enumerate([(False, False), (True, False), (True, True), (False, False)]):
        param.requires_grad_(not frozen)
        flags = step.trainable_flags()
        before = state_of(step)
        step(xn if bad else x, d, y)
        scale32 = float(E_views(step)["scale"])
        ref = G.guard_ref(before["p"], step.flat_grad.cpu(), before["m"], before["v"], steps, slots, flags, max_grad_norm=1e30,
                          skip_nonfinite=True, scale32=scale32)
        assert ref["ok"] == (not bad) and int(E_views(step)["ok"]) == int(ref["ok"])
        steps = ref["steps"]
        assert step.slot_steps_dev.tolist() == steps
        if bad:
            assert_same_state(before, state_of(step))
        else:
            check_slots(f"step {it}", ref, step.flat_param, step.exp_avg, step.exp_avg_sq, before["p"], slots)
            if frozen:
                o, n = slots[k]
                for key, t in (("p", step.flat_param), ("m", step.exp_avg), ("v", step.exp_avg_sq)):
                    assert same_bits(t[o:o + n].cpu(), before[key][o:o + n]), key
    assert steps[k] == 2 and all(s == 3 for i, s in enumerate(steps) if i != k) and step.skipped_steps() == 1
    assert_finite(step, net)


# ------------------------------------------------------------------------------------------------ 5. through RCCL
def test_guarded_trainstep_distributed_world1_bit_identical():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               C2S_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guard_dist_worker.py")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "GUARD_DIST_OK rank 0 world 1" in r.stdout
