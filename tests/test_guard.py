"""CPU checks of the guarded optimiser step's host side: the slot-table builder against TrainStep's flat layout, and the float64
reference tests/guard_ref.py against torch itself -- its clip part against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam,
its skip part against simply not calling optimizer.step(), with one parameter frozen across the skipped step."""
import numpy as np
import pytest
import torch

import guard_ref as G
from crop2seg_amd.learning.utils import slot_table

# guard_ref hands Adam grad_scale * coef rounded to float32, as the kernels do; torch multiplies by the float64 coefficient.
# That is a relative 2^-24 on every gradient, so 2^-24 on m and 2^-23 on v: the comparison below allows 4 * 2^-24.
SCALE_ROUNDING = 4 * 2.0 ** -24


def close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def layout(sizes):
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += (s + 3) // 4 * 4
    return offs, o


def test_slot_table_matches_the_flat_layout():
    sizes = [1, 3, 255, 257, 4, 2048 * 2 + 3, 8]
    offs, total = layout(sizes)
    flags = [True, True, False, True, False, True, True]
    table, mask = slot_table(offs, total, flags)
    assert [o for o, _ in table] == offs
    assert [ln for _, ln in table] == [(s + 3) // 4 * 4 for s in sizes]            # padded lengths: slots tile [0, total)
    assert all(o + ln == nxt for (o, ln), nxt in zip(table, offs[1:] + [total]))
    assert mask == [1, 1, 0, 1, 0, 1, 1]
    assert slot_table(offs, total, [False] * len(sizes))[1] == [0] * len(sizes)
    with pytest.raises(ValueError):
        slot_table(offs, total, flags[:-1])
    with pytest.raises(ValueError):
        slot_table([0, 8, 4], 12, [True] * 3)


def test_slot_table_is_what_trainstep_lays_out():
    """TrainStep's own offsets (16-byte aligned slots in named_parameters order) through the builder, without a GPU: the
    layout code of the constructor restated on a small module."""
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5), torch.nn.Linear(7, 3))
    named = list(net.named_parameters())
    named[2][1].requires_grad_(False)
    offs, total = layout([p.numel() for _, p in named])
    table, mask = slot_table(offs, total, [p.requires_grad for _, p in named])
    for (off, ln), (_, p) in zip(table, named):
        assert off % 4 == 0 and ln % 4 == 0 and p.numel() <= ln < p.numel() + 4
    assert mask == [1, 1, 0, 1, 1, 1] and table[-1][0] + table[-1][1] == total


def make_params(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=gen).double()) for s in sizes], gen


def flat(tensors, offs, total):
    out = torch.zeros(total, dtype=torch.float64)
    for t, o in zip(tensors, offs):
        out[o:o + t.numel()] = t.detach().reshape(-1)
    return out


HP = dict(lr=float(np.float32(1e-3)), betas=(float(np.float32(0.9)), float(np.float32(0.999))), eps=float(np.float32(1e-8)))


@pytest.mark.parametrize("sizes,max_norm,gmul", [([5, 300, 17], 0.5, 1.0), ([1, 3, 255, 257], 2.0, 3.0), ([64], 100.0, 1.0),
                                                 ([9, 33], 1e-3, 50.0)])
def test_guard_ref_clip_is_clip_grad_norm_then_adam(sizes, max_norm, gmul):
    params, gen = make_params(sizes, 11)
    opt = torch.optim.Adam(params, **HP)
    offs, total = layout(sizes)
    slots = [(o, s) for o, s in zip(offs, sizes)]
    flags = [True] * len(sizes)
    p, m, v = flat(params, offs, total), torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    steps = [0] * len(sizes)
    clipped = 0
    for it in range(4):
        grads = [(torch.randn(s, generator=gen) * gmul).float() for s in sizes]
        for q, gr in zip(params, grads):
            q.grad = gr.double()
        tn = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2)
        opt.step()
        r = G.guard_ref(p, flat(grads, offs, total).float(), m, v, steps, slots, flags, max_grad_norm=max_norm, bounds=False)
        assert r["ok"] and abs(r["norm"] - float(tn)) <= 1e-12 * float(tn)
        assert abs(r["coef"] - min(1.0, float(np.float32(max_norm)) / (float(tn) + 1e-6))) <= 1e-15
        clipped += r["coef"] < 1.0
        p, m, v, steps = r["p"], r["m"], r["v"], r["steps"]
        assert close(p, flat(params, offs, total), SCALE_ROUNDING)
        assert close(m, flat([opt.state[q]["exp_avg"] for q in params], offs, total), SCALE_ROUNDING)
        assert close(v, flat([opt.state[q]["exp_avg_sq"] for q in params], offs, total), SCALE_ROUNDING)
    assert steps == [4] * len(sizes)
    assert clipped == (0 if max_norm == 100.0 else 4)                      # the rows cover "clips" and "does not clip"


def test_guard_ref_skip_is_not_calling_step_with_a_parameter_frozen_across_it():
    """Steps 1-2 all trainable, step 3 non-finite with parameter 1 frozen (skipped), step 4 parameter 1 still frozen, steps 5-6
    all trainable again.  torch: the frozen parameter has grad None (Adam passes over it, its step count stays), and on the
    non-finite step optimizer.step() is not called."""
    sizes = [6, 130, 3]
    params, gen = make_params(sizes, 5)
    opt = torch.optim.Adam(params, **HP)
    offs, total = layout(sizes)
    slots = [(o, s) for o, s in zip(offs, sizes)]
    p, m, v = flat(params, offs, total), torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    steps, skipped = [0, 0, 0], 0
    for it in range(6):
        frozen = it in (2, 3)
        bad = it == 2
        flags = [True, not frozen, True]
        grads = [torch.randn(s, generator=gen).float() for s in sizes]
        if bad:
            grads[0][2] = float("inf") if it % 2 == 0 else float("nan")
        for q, gr, f in zip(params, grads, flags):
            q.grad = gr.double() if f else None
        if not bad:
            opt.step()
        before = (p.clone(), m.clone(), v.clone(), list(steps))
        r = G.guard_ref(p, flat(grads, offs, total).float(), m, v, steps, slots, flags, skip_nonfinite=True, bounds=False)
        skipped += r["skipped"]
        p, m, v, steps = r["p"], r["m"], r["v"], r["steps"]
        if bad:
            assert not r["ok"] and r["coef"] == 1.0
            assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2]) and steps == before[3]
        assert close(p, flat(params, offs, total), 1e-12)
        assert close(m, flat([opt.state[q]["exp_avg"] for q in params], offs, total), 1e-12)
        assert close(v, flat([opt.state[q]["exp_avg_sq"] for q in params], offs, total), 1e-12)
        assert steps == [int(opt.state[q]["step"]) for q in params]
    assert skipped == 1 and steps == [5, 4, 5]


def test_guard_ref_mixed_state():
    """max_grad_norm without skip_nonfinite applies a non-finite step (NaN, as today); a frozen slot full of NaN is not read."""
    slots, flags = [(0, 4), (4, 4), (8, 4)], [True, False, True]
    g = torch.ones(12)
    g[4:8] = float("nan")
    z = torch.zeros(12)
    r = G.guard_ref(z, g, z, z, [0, 7, 0], slots, flags, max_grad_norm=1.0, skip_nonfinite=True, bounds=False)
    assert r["ok"] and abs(r["norm"] - 8 ** 0.5) < 1e-15 and r["steps"] == [1, 7, 1]
    assert bool((r["p"][4:8] == 0).all()) and bool((r["p"][:4] != 0).all())
    g[0] = float("inf")
    r = G.guard_ref(z, g, z, z, [0, 7, 0], slots, flags, max_grad_norm=1.0, skip_nonfinite=False, bounds=False)
    assert r["ok"] and r["steps"] == [1, 7, 1] and not bool(torch.isfinite(r["p"][:4]).all())
    assert G.sumsq_ref(np.full(8, 1e30, np.float32), [(0, 8)], [True])[0] == pytest.approx(8e60, rel=1e-6)
