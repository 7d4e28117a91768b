"""Learning-rate schedule, parameter groups and weight decay on the GPU (csrc/guard.hip: c2s_lr_advance, c2s_adam_slots_hp;
TrainStep(lr_schedule=, weight_decay=, decoupled_weight_decay=, param_groups=)): the two entry points against numpy /
tests/optim_ref.py on a slot layout with every edge of the guarded step's, then TrainStep on U-TAE -- defaults untouched, a
schedule against the existing path with the rate poked on the host, replay, the step against the reference, skip and freeze,
set_lr_scale, resume.

Bars.  lr_now: bit for bit (one product in float64, rounded once).  Adam: the per-element bound C_BOUND * u * A of
tests/optim_ref.py (tests/tail_ref.py's conventions), tail_ref.ADAM_FROB and adam_upd_frob; the reference is fed the device's own
previous state, its published lr_now and the float32 gradient scale, so nothing accumulates.  Everything else: bit for bit."""
import numpy as np
import pytest
import torch

import optim_ref as OR
import tail_ref as R
from tail_ref import assert_within

pytestmark = pytest.mark.gpu

CHUNK = 2048                  # floats one workgroup pass covers (GD_CHUNK of csrc/guard.hip)
NAN = float("nan")
# the edges of tests/test_guard_gpu.py's SMALL: lengths 1, 3, 255, 257 (frozen, between trainable slots), 5, 2048 + 3 (from 2044
# to 4095: it straddles the chunk boundary at 2048 and ends just in front of the one at 4096, which starts in padding) and 300;
# padding behind the last slot
SLOTS = [(0, 1), (4, 3), (8, 255), (264, 257), (524, 5), (2044, CHUNK + 3), (4100, 300)]
FLAGS = [True, True, True, False, True, True, True]
TOTAL = 4403
STEPS = [1, 2, 10, 7, 1000, 1000, 2]                    # the step each slot takes (the frozen one stays at 7)
MULTS = [1.0, 0.1, 3.0, 1.0, 0.0, 1.0, 3.0]
DECAYS = [0.3, 1e-2, 0.0, 0.3, 0.3, 1e-2, 0.3]


def _E():
    from crop2seg_amd import engine as E
    return E


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


def f32bits(x):
    return int(np.float32(x).view(np.int32))


class Dev:
    """The slot layout on the device with everything the entry points take."""

    def __init__(self, steps, mults=None, decays=None, table=(1e-3,), scale=1.0, t=0, with_status=False):
        E = _E()
        self.slots = torch.tensor(SLOTS, device="cuda", dtype=torch.int64)
        self.mask = torch.tensor([1 if f else 0 for f in FLAGS], device="cuda", dtype=torch.int32)
        self.steps = torch.tensor(steps, device="cuda", dtype=torch.int32)
        hp = list(zip(mults or [1.0] * len(SLOTS), decays or [0.0] * len(SLOTS)))
        self.hp = torch.tensor(hp, dtype=torch.float32).cuda()
        self.table = torch.tensor(table, dtype=torch.float32).cuda()
        self.sched = E.sched_state("cuda", t, scale)
        self.sv = E.sched_views(self.sched)
        self.status = E.guard_status("cuda") if with_status else None
        self.gv = E.guard_views(self.status) if with_status else None
        self.skip = torch.zeros(1, device="cuda", dtype=torch.int32)
        self.ws = E.Workspace(torch.device("cuda"))

    def decide(self, ok, scale=1.0):
        """What c2s_step_decide would leave in the status block, written by the test."""
        self.gv["ok"].fill_(1 if ok else 0)
        self.gv["scale"].fill_(scale)


def inside():
    m = torch.zeros(TOTAL, dtype=torch.bool)
    for (o, n), f in zip(SLOTS, FLAGS):
        if f:
            m[o:o + n] = True
    return m


def adam_state(seed):
    """p, g, m, v float32 [TOTAL]: random inside the trainable slots, NaN in the frozen slot and in all padding."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(TOTAL, generator=gen) * 1e-2
    g = torch.randn(TOTAL, generator=gen)
    m = torch.randn(TOTAL, generator=gen) * 0.1
    v = torch.rand(TOTAL, generator=gen) * 0.01
    out = ~inside()
    for t in (p, g, m, v):
        t[out] = NAN
    return p, g, m, v


# ------------------------------------------------------------------------------------------------ 1. c2s_lr_advance
LR_TABLE = [3e-4, 1e-3, 1e-2, 4e-8]


@pytest.mark.parametrize("scale", [1.0, 0.1])
@pytest.mark.parametrize("with_status", [False, True], ids=["unguarded", "status"])
def test_lr_advance(scale, with_status):
    E = _E()
    steps0 = [0, 3, 9, 7, 999, 99999, 1]
    d = Dev(steps0, table=LR_TABLE, scale=scale, with_status=with_status)
    raw0 = bits(d.sched).clone()
    assert raw0.tolist() == [0, f32bits(scale), 0, 0]
    t, steps = 0, list(steps0)
    for k in range(6):
        applied = not (with_status and k == 2)                   # one skipped step in the middle
        if with_status:
            d.decide(applied)
        before = bits(d.sched).clone()
        E.lr_advance(d.sched, d.table, d.mask, d.steps, d.status)
        if applied:
            want = OR.lr_now_ref(LR_TABLE, t, scale)
            t += 1
            if not with_status:                                 # nobody else counts an unguarded step
                steps = [s + 1 if f else s for s, f in zip(steps, FLAGS)]
            got = bits(d.sched).tolist()
            print(f"  call {k}: t {got[0]} lr_now {float(d.sv['lr_now'])!r} want {want!r}")
            assert got == [t, f32bits(scale), f32bits(want), 0]
        else:
            assert same_bits(d.sched, before)
        assert int(d.sv["t"]) == t and d.steps.tolist() == steps     # with a status the counts are step_decide's to advance
    assert t == (5 if with_status else 6)
    assert float(d.sv["lr_now"]) == OR.lr_now_ref(LR_TABLE, 3, scale)      # past its end the table holds its last entry


# ------------------------------------------------------------------------------------------------ 2. c2s_adam_slots_hp
def check_slots(what, refs, got_p, got_m, got_v, p0):
    worst = 0.0
    for i, (o, A) in refs.items():
        off, n = SLOTS[i]
        s = slice(off, off + n)
        for name, got in (("m", got_m), ("v", got_v), ("p", got_p)):
            worst = max(worst, assert_within(f"{what} slot {i} {name}", got[s].cpu(), o[name], A[name], R.C_BOUND, R.ADAM_FROB))
        upd = got_p[s].double().cpu() - p0[s].double().cpu()
        worst = max(worst, assert_within(f"{what} slot {i} upd", upd, o["upd"], A["upd"], R.C_BOUND, R.adam_upd_frob(o, A)))
    return worst


@pytest.mark.parametrize("with_status", [False, True], ids=["unguarded", "status"])
@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_adam_slots_hp_against_adam_hp_ref(decoupled, gs, with_status):
    E = _E()
    table = [2e-3, 1e-3]
    steps = [s - 1 if f else s for s, f in zip(STEPS, FLAGS)]
    d = Dev(steps, MULTS, DECAYS, table=table, with_status=with_status)
    p, g, m, v = adam_state(31)
    pd, gd, md, vd = p.cuda(), g.cuda(), m.cuda(), v.cuda()
    out = ~inside()
    for it in range(2):                                          # the second step starts from the device's own state
        p0, m0, v0 = pd.cpu(), md.cpu(), vd.cpu()
        if with_status:
            d.decide(True, gs)
            d.steps += d.mask                                    # c2s_step_decide's part
        E.lr_advance(d.sched, d.table, d.mask, d.steps, d.status)
        E.adam_slots_hp(pd, gd, md, vd, d.slots, d.mask, d.steps, d.hp, d.sched, d.status, decoupled=decoupled,
                        grad_scale=777.0 if with_status else gs)          # ignored where a status decides
        lr_now = float(d.sv["lr_now"])
        assert lr_now == OR.lr_now_ref(table, it) and int(d.sv["t"]) == it + 1
        now = [s + it for s in STEPS]
        assert d.steps.tolist() == [n if f else s for n, s, f in zip(now, STEPS, FLAGS)]
        refs = {}
        for i, ((o, n), f) in enumerate(zip(SLOTS, FLAGS)):
            if f:
                s = slice(o, o + n)
                refs[i] = OR.adam_hp_ref(p0[s], g[s], m0[s], v0[s], now[i], lr_now, MULTS[i], DECAYS[i], decoupled, grad_scale=gs)
        worst = check_slots(f"step {it}", refs, pd, md, vd, p0)
        print(f"  decoupled {decoupled} gs {gs} step {it}: worst ratio {worst:.3f}")
        for name, got, was in (("p", pd, p), ("m", md, m), ("v", vd, v)):     # frozen slot and padding keep their NaN bits
            assert same_bits(got.cpu()[out], was[out]), name
        assert same_bits(gd.cpu(), g)
        o4, n4 = SLOTS[4]                                        # multiplier 0: p keeps its bits, m and v advance
        assert same_bits(pd[o4:o4 + n4].cpu(), p0[o4:o4 + n4])
        assert not same_bits(md[o4:o4 + n4].cpu(), m0[o4:o4 + n4]) and not same_bits(vd[o4:o4 + n4].cpu(), v0[o4:o4 + n4])
        o5, n5 = SLOTS[5]
        assert not same_bits(pd[o5:o5 + n5].cpu(), p0[o5:o5 + n5])


def test_adam_slots_hp_decay_forms_differ_and_decay_matters():
    """The three arithmetic branches are three results: no decay, coupled and decoupled differ on a decayed slot."""
    E = _E()
    res = []
    for decays, decoupled in ((None, False), (DECAYS, False), (DECAYS, True)):
        d = Dev([9] * len(SLOTS), MULTS, decays, table=[1e-2])
        a = [x.cuda() for x in adam_state(32)]
        E.lr_advance(d.sched, d.table, d.mask, d.steps)
        E.adam_slots_hp(*a, d.slots, d.mask, d.steps, d.hp, d.sched, decoupled=decoupled)
        res.append(a[0][2044:2044 + CHUNK + 3].cpu())
    assert not same_bits(res[0], res[1]) and not same_bits(res[0], res[2]) and not same_bits(res[1], res[2])


# ------------------------------------------------------------------------------------------------ 3. neutral settings
@pytest.mark.parametrize("step,gs", [(1, 1.0), (1000, 0.5)])
def test_neutral_settings_equal_adam_slots_and_adam_flat(step, gs):
    """Table [lr], multipliers 1, decays 0: the bits of c2s_adam_slots (status given) and of c2s_adam_flat over the trainable
    runs (status NULL)."""
    E = _E()
    lr = 1e-3
    p, g, m, v = adam_state(33)
    # status given
    a = [x.cuda() for x in (p, g, m, v)]
    b = [x.cuda() for x in (p, g, m, v)]
    da = Dev([step - 1] * len(SLOTS), with_status=True)
    db = Dev([step - 1] * len(SLOTS), table=[lr], with_status=True)
    for d in (da, db):
        E.grad_sumsq(a[1], d.slots, d.mask, d.ws, d.status)
        E.step_decide(d.status, None, gs, True, d.mask, d.steps, d.skip)
    E.adam_slots(*a, da.slots, da.mask, da.steps, da.status, lr)
    E.lr_advance(db.sched, db.table, db.mask, db.steps, db.status)
    E.adam_slots_hp(*b, db.slots, db.mask, db.steps, db.hp, db.sched, db.status)
    assert da.steps.tolist() == db.steps.tolist() == [step if f else step - 1 for f in FLAGS]
    for x, y, name in zip(a, b, "pgmv"):
        assert same_bits(x, y), name
    assert not same_bits(a[0].cpu()[inside()], p[inside()])
    # status NULL
    c = [x.cuda() for x in (p, g, m, v)]
    e = [x.cuda() for x in (p, g, m, v)]
    dc = Dev([step - 1] * len(SLOTS), table=[lr])
    E.lr_advance(dc.sched, dc.table, dc.mask, dc.steps)
    E.adam_slots_hp(*c, dc.slots, dc.mask, dc.steps, dc.hp, dc.sched, grad_scale=gs)
    for (o, n), f in zip(SLOTS, FLAGS):
        if f:
            E.adam_flat(*[x[o:o + n] for x in e], step, lr, grad_scale=gs)
    for x, y, name in zip(c, e, "pgmv"):
        assert same_bits(x, y), name
    for x, y, name in zip(b, c, "pgmv"):
        assert same_bits(x, y), name


# ------------------------------------------------------------------------------------------------ 4. skipped step
def test_skipped_step_writes_nothing():
    E = _E()
    steps = [3, 1, 9, 4, 999, 99999, 1]
    d = Dev(steps, MULTS, DECAYS, table=LR_TABLE, scale=0.5, t=2, with_status=True)
    p, g, m, v = adam_state(34)
    a = [x.cuda() for x in (p, g, m, v)]
    raw = bits(d.sched).clone()
    d.decide(False, 0.25)
    for decoupled in (False, True):
        E.lr_advance(d.sched, d.table, d.mask, d.steps, d.status)
        E.adam_slots_hp(*a, d.slots, d.mask, d.steps, d.hp, d.sched, d.status, decoupled=decoupled)
    assert same_bits(d.sched, raw) and d.steps.tolist() == steps
    for x, y, name in zip(a, (p, g, m, v), "pgmv"):
        assert same_bits(x.cpu(), y), name


# ------------------------------------------------------------------------------------------------ TrainStep on U-TAE
def fresh(**kw):
    """U-TAE in the seeded "tame" state, dropout off, and its TrainStep (the set-up of tests/test_guard_gpu.py)."""
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
    if callable(kw.get("feature")):
        kw.update(kw.pop("feature")(net))
    return net, TrainStep(net, num_classes=15, **kw)


_BATCH = {}


def batch():
    from oracle import seeded
    if not _BATCH:
        x, dates, y = seeded.make_inputs(2, 4, 10, 32, 32, 91, [4, 3])
        _BATCH["dev"] = (x.cuda(), dates.cuda(), y.cuda())
        xn = x.clone()
        xn[1, 2, 3, 17, 5] = NAN                                   # one NaN pixel
        _BATCH["nan"] = (xn.cuda(), dates.cuda(), y.cuda())
    return _BATCH


ENCODER = ("in_conv.", "down_blocks.")
WEIGHT = "in_conv.conv.conv.0.weight"                             # an encoder weight: multiplier 0.1, decayed


def feature(net, decoupled=True, table=None):
    """warmup_cosine over 8 steps, the encoder at multiplier 0.1, norm gains and biases undecayed, global decay 1e-2.  A
    parameter may be in one group only, so the encoder's gains and biases form a group of their own."""
    from crop2seg_amd.learning import schedules as S
    nd = set(S.no_decay_names(net))
    names = [n for n, _ in net.named_parameters()]
    groups = [{"params": [n for n in names if n.startswith(ENCODER) and n not in nd], "lr_mult": 0.1},
              {"params": [n for n in names if n.startswith(ENCODER) and n in nd], "lr_mult": 0.1, "weight_decay": 0},
              {"params": lambda n: n in nd and not n.startswith(ENCODER), "weight_decay": 0}]
    return dict(lr_schedule=table or S.warmup_cosine(1e-3, 3, 8), param_groups=groups, weight_decay=1e-2,
                decoupled_weight_decay=decoupled)


def state_of(step):
    s = {"p": step.flat_param, "m": step.exp_avg, "v": step.exp_avg_sq}
    if getattr(step, "flat_buf", None) is not None:
        s["buf"] = step.flat_buf
    if getattr(step, "slot_steps_dev", None) is not None:
        s["steps"] = step.slot_steps_dev
    if step.hp:
        s["sched"] = step.sched_dev
    return {k: t.detach().cpu().clone() for k, t in s.items()}


def assert_same_state(a, b, keys=None):
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and bool((a[k].view(torch.int32) == b[k].view(torch.int32)).all()), k


def assert_same_buffers(net_a, net_b):
    for (k, a), (_, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(a, b), k


GUARD = dict(max_grad_norm=1e30, skip_nonfinite=True)


def test_trainstep_defaults_launch_nothing_new(monkeypatch):
    """5. The new arguments at their defaults: no new entry point runs, three steps bit-identical to a twin built without them."""
    E = _E()
    x, d, y = batch()["dev"]
    net_a, step_a = fresh()
    for _ in range(3):
        step_a(x, d, y)

    def forbidden(*a, **k):
        raise AssertionError("a schedule entry point ran in a step built without the feature")

    for name in ("lr_advance", "adam_slots_hp", "sched_state"):
        monkeypatch.setattr(E, name, forbidden)
    net_b, step_b = fresh(lr_schedule=None, schedule_steps=None, weight_decay=0.0, decoupled_weight_decay=False,
                          param_groups=None)
    assert not step_b.hp and not step_b.guarded
    for _ in range(3):
        step_b(x, d, y)
    assert_same_state(state_of(step_a), state_of(step_b))
    assert_same_buffers(net_a, net_b)
    with pytest.raises(RuntimeError, match="no schedule"):
        step_b.schedule_position()
    with pytest.raises(RuntimeError, match="no schedule"):
        step_b.set_lr_scale(0.5)


@pytest.mark.parametrize("guard", [{}, GUARD], ids=["unguarded", "guarded"])
def test_trainstep_schedule_equals_the_rate_poked_on_the_host(guard):
    """6. lr_schedule=[a, b, c, d] against the default path with step.lr set before each eager call."""
    x, d, y = batch()["dev"]
    table = [3e-4, 1e-3, 1e-2, 4e-5]
    net_s, step_s = fresh(lr_schedule=table, **guard)
    net_h, step_h = fresh(**guard)
    assert step_s.hp and not step_h.hp
    for k, lr in enumerate(table):
        step_h.lr = lr
        lh, _ = step_h(x, d, y)
        ls, _ = step_s(x, d, y)
        assert float(lh) == float(ls), k
        assert float(step_s.last_lr) == float(np.float32(lr))
        assert_same_state(state_of(step_h), state_of(step_s), ("p", "m", "v"))
    assert_same_buffers(net_h, net_s)
    assert step_s.schedule_position() == 4 and step_s.slot_steps_dev.tolist() == [4] * len(step_s.names)


_RUNS = {}


def six_eager_steps(guarded):
    """The uninterrupted eager run of cases 7 and 11, made once: the state after six steps and a snapshot's state after three."""
    if guarded not in _RUNS:
        x, d, y = batch()["dev"]
        net, step = fresh(feature=feature, **(GUARD if guarded else {}))
        lrs, snap = [], None
        for k in range(6):
            loss, _ = step(x, d, y)
            lrs.append(float(step.last_lr))
            if k == 2:
                snap = step.snapshot().state_dict()
        _RUNS[guarded] = {"state": state_of(step), "loss": float(loss), "lrs": lrs, "snap": snap,
                          "buffers": {k: v.detach().cpu().clone() for k, v in net.state_dict().items()},
                          "table": list(step.lr_table), "position": step.schedule_position()}
    return _RUNS[guarded]


@pytest.mark.parametrize("guarded", [False, True], ids=["unguarded", "guarded"])
def test_trainstep_replay_moves_the_rate(guarded):
    """7. Three eager steps, capture(), three replays against six eager steps: the rate moves under replay."""
    x, d, y = batch()["dev"]
    want = six_eager_steps(guarded)
    table = want["table"]
    assert want["lrs"] == [float(np.float32(v)) for v in table[:6]]
    assert len(set(want["lrs"][3:])) == 3 and len(set(want["lrs"][:3])) == 3      # the replayed entries differ from one another
    net, step = fresh(feature=feature, **(GUARD if guarded else {}))
    for _ in range(3):
        step(x, d, y)
    step.capture(x, d, y)
    assert step.schedule_position() == 3                          # the warm-up pass of capture() is no step
    for k in range(3, 6):
        loss, _ = step.replay()
        assert float(step.last_lr) == float(np.float32(table[k])), k
    torch.cuda.synchronize()
    assert float(loss) == want["loss"]
    assert_same_state(want["state"], state_of(step))
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), want["buffers"][k]), k
    assert step.schedule_position() == want["position"] == 6
    assert not hasattr(step, "step_dev")


def slots_of(step):
    from crop2seg_amd.learning.utils import slot_table
    return slot_table(step.offsets, step.total, [True] * len(step.offsets))[0]


@pytest.mark.parametrize("clip", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_trainstep_against_adam_hp_ref(decoupled, clip):
    """8. Every parameter's update within the per-element bounds of adam_hp_ref, fed flat_grad, the previous state, the slot
    steps and the published lr_now; clipped: max_grad_norm = half the first gradient's norm, so coef < 1."""
    E = _E()
    x, d, y = batch()["dev"]
    kw = {}
    if clip:
        _, probe = fresh()
        probe(x, d, y, apply_update=False)
        kw["max_grad_norm"] = 0.5 * float(probe.flat_grad.double().norm())
    net, step = fresh(feature=lambda n: feature(n, decoupled), **kw)
    slots = slots_of(step)
    assert any(w > 0 and a != 1 for a, w in step.slot_hp) and any(w == 0 for _, w in step.slot_hp)
    for it in range(2):
        before = state_of(step)
        step(x, d, y)
        g = step.flat_grad.cpu()
        gs = 1.0
        if clip:
            views = E.guard_views(step._status)
            gs = float(views["scale"])
            assert float(views["coef"]) < 1.0, "clipping is not active"
        lr_now = float(step.last_lr)
        assert lr_now == OR.lr_now_ref(step.lr_table, it)
        assert step.slot_steps_dev.tolist() == [it + 1] * len(slots)
        worst = 0.0
        for i, (o, n) in enumerate(slots):
            s = slice(o, o + n)
            mult, wd = step.slot_hp[i]
            ref, A = OR.adam_hp_ref(before["p"][s], g[s], before["m"][s], before["v"][s], it + 1, lr_now, mult, wd, decoupled,
                                    grad_scale=gs)
            what = f"step {it} {step.names[i]}"
            for name, got in (("m", step.exp_avg), ("v", step.exp_avg_sq), ("p", step.flat_param)):
                worst = max(worst, assert_within(f"{what} {name}", got[s].cpu(), ref[name], A[name], R.C_BOUND, R.ADAM_FROB))
            upd = step.flat_param[s].double().cpu() - before["p"][s].double()
            worst = max(worst, assert_within(f"{what} upd", upd, ref["upd"], A["upd"], R.C_BOUND, R.adam_upd_frob(ref, A)))
        print(f"  decoupled {decoupled} clip {clip} step {it}: lr_now {lr_now!r} scale {gs!r} worst ratio {worst:.3f}")


def test_trainstep_skip_and_freeze():
    """9. A NaN batch under skip_nonfinite: position, rate, parameters and moments stay, and the next good step takes the entry
    the skipped one would have taken.  A parameter frozen for two steps keeps its bits through decoupled decay."""
    x, d, y = batch()["dev"]
    xn, _, _ = batch()["nan"]
    net, step = fresh(feature=feature, skip_nonfinite=True)
    table = step.lr_table
    step(x, d, y)
    before = state_of(step)
    assert step.schedule_position() == 1 and float(step.last_lr) == float(np.float32(table[0]))
    step(xn, d, y)
    assert step.skipped_steps() == 1 and step.schedule_position() == 1
    assert_same_state(before, state_of(step))                     # sched (t, scale, lr_now), steps, p, m, v, buffers
    step(x, d, y)
    assert step.schedule_position() == 2 and float(step.last_lr) == float(np.float32(table[1]))
    after = state_of(step)
    assert not torch.equal(after["p"], before["p"]) and (after["steps"] == before["steps"] + 1).all()
    # freeze
    k = step.names.index(WEIGHT)
    assert step.slot_hp[k][1] > 0 and step.decoupled
    o, n = slots_of(step)[k]
    param = dict(net.named_parameters())[WEIGHT]
    param.requires_grad_(False)
    for _ in range(2):
        step(x, d, y)
    frozen = state_of(step)
    for key in ("p", "m", "v"):
        assert same_bits(frozen[key][o:o + n], after[key][o:o + n]), key
    assert int(frozen["steps"][k]) == 2 and step.schedule_position() == 4
    assert not same_bits(frozen["p"][o + n:], after["p"][o + n:])
    param.requires_grad_(True)
    step(x, d, y)
    last = state_of(step)
    assert not same_bits(last["p"][o:o + n], frozen["p"][o:o + n]) and int(last["steps"][k]) == 3


def test_trainstep_set_lr_scale_between_replays(monkeypatch):
    """10. set_lr_scale(0.1) between replays: the next replay's rate is float32(table[t] * 0.1), the step an eager twin's."""
    x, d, y = batch()["dev"]
    net_r, step_r = fresh(feature=feature)
    net_e, step_e = fresh(feature=feature)
    table = step_r.lr_table
    step_r.capture(x, d, y)
    for step, run in ((step_r, step_r.replay), (step_e, lambda: step_e(x, d, y))):
        run()
        assert float(step.last_lr) == float(np.float32(table[0]))
        step.set_lr_scale(0.1)
        run()
        want = OR.lr_now_ref(table, 1, 0.1)
        assert float(step.last_lr) == want and want != float(np.float32(table[1]))
        run()
        assert float(step.last_lr) == OR.lr_now_ref(table, 2, 0.1)
    torch.cuda.synchronize()
    assert_same_state(state_of(step_e), state_of(step_r))
    assert_same_buffers(net_e, net_r)
    with pytest.raises(ValueError):
        step_r.set_lr_scale(-1.0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        step_r.set_lr_scale(0.5)


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_trainstep_resume(mode):
    """11. The snapshot after step 3 of 6 into a fresh twin: after step 6 it is the uninterrupted run bit for bit."""
    x, d, y = batch()["dev"]
    want = six_eager_steps(False)
    net, step = fresh(feature=feature)
    info = step.load_state_dict(want["snap"])
    assert info["bit_exact"] and info["schedule_bit_exact"] and not any(info["optim_differs"].values())
    assert step.schedule_position() == 3 and float(step.last_lr) == want["lrs"][2]
    if mode == "captured":
        step.capture(x, d, y)
    for _ in range(3):
        loss, _ = step.replay() if mode == "captured" else step(x, d, y)
    torch.cuda.synchronize()
    assert float(loss) == want["loss"]
    assert_same_state(want["state"], state_of(step))
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), want["buffers"][k]), k
    assert step.schedule_position() == 6


def test_trainstep_resume_other_table_and_feature_off():
    """11. A twin with another table loads, continues from the same position and is told that the schedule differs; a twin
    without the feature refuses the state and changes nothing; a state written without the feature loads at t = its steps."""
    x, d, y = batch()["dev"]
    want = six_eager_steps(False)
    other = [5e-4] * 8
    net, step = fresh(feature=lambda n: feature(n, table=other))
    info = step.load_state_dict(want["snap"])
    assert info["optim_differs"] == {"schedule": True, "groups": False, "mode": False}
    assert step.schedule_position() == 3
    step(x, d, y)
    assert step.schedule_position() == 4 and float(step.last_lr) == float(np.float32(5e-4))
    opt = want["snap"]["optimizer"]["param_groups"]
    assert len(opt) == 1 and opt[0]["weight_decay"] == 1e-2 and opt[0]["lr"] == OR.lr_now_ref(want["table"], 3)
    # feature off
    net_o, step_o = fresh()
    step_o(x, d, y)
    before = state_of(step_o)
    with pytest.raises(ValueError, match="schedule mode"):
        step_o.load_state_dict(want["snap"])
    assert_same_state(before, state_of(step_o))
    # a state written with the feature off, into a step with it on
    step_o(x, d, y)
    plain = step_o.snapshot().state_dict()
    assert "optim" not in plain["crop2seg_amd"]
    net_n, step_n = fresh(feature=feature)
    info = step_n.load_state_dict(plain)
    assert info["optim_differs"] is None and info["schedule_bit_exact"]
    assert step_n.schedule_position() == 2 and bits(step_n.sched_dev).tolist()[1] == f32bits(1.0)
    assert_same_state(state_of(step_o), state_of(step_n), ("p", "m", "v"))
    step_n(x, d, y)
    assert float(step_n.last_lr) == float(np.float32(step_n.lr_table[2]))
