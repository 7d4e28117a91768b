"""The scheduled / grouped / decayed Adam step without a GPU: tests/optim_ref.py against torch.optim.Adam(weight_decay=) and
torch.optim.AdamW, the schedule tables of crop2seg_amd/learning/schedules.py against torch.optim.lr_scheduler, the planted
faults the comparison must catch, and the resolution of parameter groups."""
import math

import numpy as np
import pytest
import torch

import optim_ref as OR
import tail_ref as R
from crop2seg_amd.learning import schedules as S

STEPS = 40
SIZES, MULTS, DECAYS = (5, 7, 3), (1.0, 0.1, 0.0), (0.0, 1e-2, 0.3)
GROUPS = list(zip(MULTS, DECAYS))


def one_cycle():
    return S.from_torch(lambda o: torch.optim.lr_scheduler.OneCycleLR(o, max_lr=1e-2, total_steps=STEPS), 1e-3, STEPS)


def problem(seed=5, attempts=STEPS):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen, dtype=torch.float64) for n in SIZES]
    grads = [[torch.randn(n, generator=gen, dtype=torch.float64) for n in SIZES] for _ in range(attempts)]
    return params, grads


def rel_diff(a, b):
    return max(float(((x - y).abs() / y.abs().clamp_min(1e-300)).max()) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ adam_hp_ref
@pytest.mark.parametrize("step,gs", [(1, 1.0), (2, 0.25), (1000, 1.0)])
def test_adam_hp_ref_neutral_is_adam_ref(step, gs):
    gen = torch.Generator().manual_seed(step)
    p, g = torch.randn(300, generator=gen) * 1e-2, torch.randn(300, generator=gen)
    m, v = torch.randn(300, generator=gen) * 0.1, torch.rand(300, generator=gen) * 0.01
    for decoupled in (False, True):
        o, A = OR.adam_hp_ref(p, g, m, v, step, 1e-3, 1.0, 0.0, decoupled, grad_scale=gs)
        o0, A0 = R.adam_ref(p, g, m, v, step, lr=1e-3, grad_scale=gs)
        assert set(o) == set(o0) and set(A) == set(A0)
        for k in o0:
            assert torch.equal(o[k], o0[k]), k
        for k in A0:
            assert torch.equal(A[k], A0[k]), k


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_adam_hp_ref_general_path_meets_adam_ref_as_decay_vanishes(decoupled):
    """The general restatement at a decay too small to matter: values as adam_ref to float64 noise, bounds never below it."""
    gen = torch.Generator().manual_seed(9)
    p, g = torch.randn(64, generator=gen) * 1e-2, torch.randn(64, generator=gen)
    m, v = torch.randn(64, generator=gen) * 0.1, torch.rand(64, generator=gen) * 0.01
    o, A = OR.adam_hp_ref(p, g, m, v, 10, 1e-3, 1.0, 1e-30, decoupled)
    o0, A0 = R.adam_ref(p, g, m, v, 10, lr=1e-3)
    for k in ("m", "v", "p"):
        assert float((o[k] - o0[k]).abs().max()) <= 1e-15 * float(o0[k].abs().max()), k
        assert bool((A[k] >= A0[k] * (1 - 1e-12)).all()), k


# ------------------------------------------------------------------------------------------------ against torch
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam_weight_decay", "adamw"])
def test_trajectory_equals_torch(decoupled):
    params, grads = problem()
    table = one_cycle()
    ours = OR.trajectory(params, grads, table, GROUPS, decoupled)
    theirs = OR.torch_trajectory(params, grads, table, GROUPS, decoupled)
    d = rel_diff(ours, theirs)
    print(f"  decoupled {decoupled}: max relative difference {d:.3e}")
    assert d <= 1e-12
    assert torch.equal(ours[2], params[2]) and torch.equal(theirs[2], params[2])        # multiplier 0: the parameter stays
    assert rel_diff(ours[:2], params[:2]) > 1e-3


FAULTS = [("decay_on_grad_decoupled", True), ("decoupled_base_lr", True), ("no_mult", False), ("no_mult", True),
          ("table_next", False), ("advance_on_skip", True)]


@pytest.mark.parametrize("fault,decoupled", FAULTS, ids=[f"{f}-{'adamw' if d else 'adam'}" for f, d in FAULTS])
def test_planted_faults_break_the_comparison(fault, decoupled):
    """One skipped attempt in the middle (torch: no optimizer.step(), the position stays): sound it still equals torch, with
    the fault it does not."""
    params, grads = problem(seed=6, attempts=STEPS + 1)
    table, skipped = one_cycle(), (17,)
    theirs = OR.torch_trajectory(params, grads, table, GROUPS, decoupled, skipped)
    sound = rel_diff(OR.trajectory(params, grads, table, GROUPS, decoupled, skipped), theirs)
    broken = rel_diff(OR.trajectory(params, grads, table, GROUPS, decoupled, skipped, fault=fault), theirs)
    print(f"  {fault}: sound {sound:.3e} broken {broken:.3e}")
    assert sound <= 1e-12 < broken


# ------------------------------------------------------------------------------------------------ schedules
def test_from_torch_reproduces_the_schedulers():
    L = torch.optim.lr_scheduler
    cases = {"cosine": lambda o: L.CosineAnnealingLR(o, T_max=25, eta_min=1e-5),
             "multistep": lambda o: L.MultiStepLR(o, milestones=[5, 11, 30], gamma=0.3),
             "onecycle": lambda o: L.OneCycleLR(o, max_lr=1e-2, total_steps=STEPS)}
    for name, factory in cases.items():
        table = S.from_torch(factory, 1e-3, STEPS)
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=1e-3)
        sched = factory(opt)
        want = []
        for _ in range(STEPS):
            want.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        assert len(table) == STEPS and all(type(a) is float for a in table), name
        assert table == want, name
    assert S.from_torch(cases["multistep"], 1e-3, 12)[11] == pytest.approx(1e-3 * 0.09, rel=1e-12)


def test_warmup_cosine_closed_form_and_lambda_lr():
    base, warm, total, lo = 3e-3, 5, 37, 1e-5
    table = S.warmup_cosine(base, warm, total, lo)
    assert len(table) == total

    def closed(t):
        if t < warm:
            return base * (t + 1) / warm
        x = (t - warm) / (total - 1 - warm)
        return lo + (base - lo) * 0.5 * (1 + math.cos(math.pi * x))

    lam = S.from_torch(lambda o: torch.optim.lr_scheduler.LambdaLR(
        o, lambda t: S.warmup_cosine_factor(t, warm, total, lo / base)), base, total)
    for t in range(total):
        assert abs(table[t] - closed(t)) <= 1e-15 * closed(t), t
        assert abs(table[t] - lam[t]) <= 1e-15 * lam[t], t
    assert table[warm - 1] == base and table[warm] == base and abs(table[-1] - lo) <= 1e-15 * lo
    assert S.warmup_cosine(1e-3, 0, 1) == [1e-3]


def test_table_holds_its_last_entry_and_validates():
    table = S.schedule_table(1e-3, [3e-4, 1e-3, 4e-8])
    assert [S.table_at(table, t) for t in (0, 2, 3, 10 ** 9)] == [3e-4, 4e-8, 4e-8, 4e-8]
    assert OR.lr_now_ref(table, 7, 0.1) == float(np.float32(np.float64(np.float32(4e-8)) * np.float64(np.float32(0.1))))
    assert S.schedule_table(2e-3) == [2e-3]
    assert S.schedule_table(1.0, lambda t: 0.5 ** t, 3) == [1.0, 0.5, 0.25]
    for bad in ([1e-3, float("nan")], [float("inf")], [-1e-3], []):
        with pytest.raises(ValueError):
            S.schedule_table(1e-3, bad)
    with pytest.raises(ValueError):
        S.schedule_table(1e-3, lambda t: 1.0)                   # a callable needs schedule_steps
    assert S.table_digest([1e-3, 2e-3]) != S.table_digest([1e-3, 2.000001e-3]) and len(S.table_digest([1.0])) == 64


def test_no_decay_names():
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.GroupNorm(2, 4), torch.nn.Linear(4, 2, bias=False))
    assert S.no_decay_names(net) == ["0.bias", "1.weight", "1.bias"]


# ------------------------------------------------------------------------------------------------ groups
NAMES = ["enc.0.weight", "enc.0.bias", "enc.1.weight", "head.weight", "head.bias", "encoder_extra"]


def test_group_resolution():
    r = S.resolve_param_groups
    assert r(NAMES) == [(1.0, 0.0)] * 6
    assert r(NAMES, None, 0.05) == [(1.0, 0.05)] * 6
    assert r(NAMES, [{"params": "enc.", "lr_mult": 0.1}], 0.01) == [(0.1, 0.01)] * 3 + [(1.0, 0.01)] * 3
    assert r(NAMES, [{"params": "enc", "lr_mult": 0.1}], 0.01)[5] == (0.1, 0.01)                   # a prefix, not a module path
    got = r(NAMES, [{"params": ["enc.0.bias", "head.bias"], "weight_decay": 0}, {"params": lambda n: n.startswith("head.w"),
                                                                                   "lr_mult": 3}], 0.01)
    assert got == [(1.0, 0.01), (1.0, 0.0), (1.0, 0.01), (3.0, 0.01), (1.0, 0.0), (1.0, 0.01)]
    assert r(NAMES, [{"params": "head", "lr_mult": 0, "weight_decay": 0.3}])[3] == (0.0, 0.3)
    with pytest.raises(ValueError, match=r"param_groups\[1\].*matches no parameter"):
        r(NAMES, [{"params": "enc."}, {"params": "decoder."}])
    with pytest.raises(ValueError, match=r"'enc.0.bias' is matched by param_groups\[0\] and param_groups\[1\]"):
        r(NAMES, [{"params": "enc."}, {"params": ["enc.0.bias"]}])
    with pytest.raises(ValueError, match="lr_mult"):
        r(NAMES, [{"params": "enc.", "lr_mult": -0.1}])
    with pytest.raises(ValueError, match=r"param_groups\[0\]\['weight_decay'\]"):
        r(NAMES, [{"params": "enc.", "weight_decay": -1e-2}])
    with pytest.raises(ValueError, match="weight_decay"):
        r(NAMES, None, -1e-2)
    with pytest.raises(ValueError, match="unknown keys"):
        r(NAMES, [{"params": "enc.", "lr": 1e-3}])
