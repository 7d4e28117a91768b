"""float64 restatement of the scheduled, grouped, decayed Adam step (csrc/guard.hip: c2s_lr_advance, c2s_adam_slots_hp) with
per-element bounds in the conventions of tests/tail_ref.py (C_BOUND, U, POW_ULPS), and a multi-step driver that is compared with
torch.optim.Adam(weight_decay=) / torch.optim.AdamW on the CPU.

    lr_s = lr_now mult                                  one float32 rounding: the reference takes the rounded value as exact
    coupled   (torch.optim.Adam(weight_decay=wd)):  gg = g gs + wd p      A_gg  = |g gs| + |wd p| + |gg|
    decoupled (torch.optim.AdamW):                  f = 1 - lr_s wd       A_f   = |lr_s wd| + |f|
                                                    p~ = p f              A_p~  = |p| A_f + |p~|
    then tail_ref.adam_ref's arithmetic on gg / p~ with A_gg and A_p~ carried through:
        A_mm = |b1 m| + c1 (A_gg + 2 |gg|) + |mm|;  A_vv = |b2 v| + c2 (3 gg^2 + 2 |gg| A_gg) + vv;  A_p = A_s + A_p~ + |p'|
    upd = p' - p counts from the p before the decay.

With wd = 0 the step IS tail_ref.adam_ref at lr_s (the call is handed over), so outputs and bounds are that function's.

Nothing here imports crop2seg_amd or oracle.
"""
import numpy as np
import torch

import tail_ref as R
from tail_ref import POW_ULPS, _f


def f32(x):
    return float(np.float32(x))


def lr_now_ref(table, t, scale=1.0):
    """float32(float64(float32 table[min(t, n - 1)]) * float64(float32 scale)): what c2s_lr_advance publishes."""
    return f32(np.float64(np.float32(table[min(max(t, 0), len(table) - 1)])) * np.float64(np.float32(scale)))


def adam_hp_ref(p, g, m, v, step, lr_now, mult=1.0, wd=0.0, decoupled=False, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0,
                dtype=torch.float64, bounds=True, hyper32=True, fault=None):
    """One step on flat tensors; returns ({"m", "v", "p", "upd"}, bounds A).  hyper32: hyper-parameters as float32 values widened
    (what the kernel receives), lr_s rounded to float32 once; False: Python doubles throughout (the comparison with torch).

    fault: "decay_on_grad_decoupled" decoupled mode adds wd p to the gradient instead; "decoupled_base_lr" the decoupled decay
    uses lr_now without the multiplier; "no_mult" the step size is lr_now."""
    cv = f32 if hyper32 else float
    if hyper32 and cv(wd) == 0.0 and fault is None:
        return R.adam_ref(p, g, m, v, step, lr=f32(np.float32(lr_now) * np.float32(mult)), b1=b1, b2=b2, eps=eps,
                          grad_scale=grad_scale, dtype=dtype, bounds=bounds)
    bounds = bounds and dtype == torch.float64
    p, g, m, v = (_f(x, dtype).reshape(-1) for x in (p, g, m, v))
    lr_s = cv(lr_now) * cv(mult)
    if hyper32:
        lr_s = f32(np.float32(lr_now) * np.float32(mult))
    if fault == "no_mult":
        lr_s = cv(lr_now)
    lr_s, lr0, wd, b1, b2, eps, gs = (torch.tensor(x, dtype=dtype) for x in (lr_s, cv(lr_now), cv(wd), cv(b1), cv(b2), cv(eps),
                                                                              cv(grad_scale)))
    st = torch.tensor(float(step), dtype=dtype)
    gg = g * gs
    A_gg = gg.abs()
    pin, A_pin = p, torch.zeros_like(p)
    if float(wd) != 0.0:
        if decoupled and fault != "decay_on_grad_decoupled":
            q = (lr0 if fault == "decoupled_base_lr" else lr_s) * wd
            f = 1 - q
            pin = p * f
            A_pin = p.abs() * (q.abs() + f.abs()) + pin.abs()
        else:
            wp = wd * p
            gg = gg + wp
            A_gg = A_gg + wp.abs() + gg.abs()
    c1, c2 = 1 - b1, 1 - b2
    mm = b1 * m + c1 * gg
    vv = b2 * v + c2 * gg * gg
    pw1, pw2 = torch.pow(b1, st), torch.pow(b2, st)
    bc1, bc2 = 1 - pw1, 1 - pw2
    rb = torch.sqrt(bc2)
    sq = torch.sqrt(vv)
    den = sq / rb + eps
    a = lr_s / bc1
    r = mm / den
    s = a * r
    pn = pin - s
    out = {"m": mm, "v": vv, "p": pn, "upd": pn - p}
    if not bounds:
        return out, {}
    A_mm = (b1 * m).abs() + c1 * (A_gg + 2 * gg.abs()) + mm.abs()
    A_vv = (b2 * v).abs() + c2 * (3 * gg * gg + 2 * gg.abs() * A_gg) + vv
    A_bc1 = 2 * POW_ULPS * pw1 + bc1
    A_rb = (2 * POW_ULPS * pw2 + bc2) / (2 * rb) + rb
    A_sq = torch.where(sq > 0, A_vv / (2 * sq.clamp_min(1e-300)), torch.zeros_like(sq)) + sq
    A_den = A_sq / rb + sq * A_rb / rb ** 2 + sq / rb + den
    A_a = lr_s * A_bc1 / bc1 ** 2 + a
    A_r = A_mm / den + mm.abs() * A_den / den ** 2 + r.abs()
    A_s = A_a * r.abs() + a * A_r + s.abs()
    A_p = A_s + A_pin + pn.abs()
    return out, {"m": A_mm, "v": A_vv, "p": A_p, "upd": A_p, "bc_rel": A_bc1 / bc1 + A_rb / rb}


def trajectory(params, grads, table, groups, decoupled, skipped=(), b1=0.9, b2=0.999, eps=1e-8, fault=None):
    """The restated run in Python doubles: params = one float64 tensor per group, grads[k] = their gradients at attempt k,
    groups = (lr_mult, weight_decay) per group, skipped = the attempts whose step is not applied.  The rate of an applied step is
    table[min(t, n - 1)] with t the number of steps applied before it.  Returns the parameters after the last attempt.

    fault: those of adam_hp_ref, "table_next" (table[t + 1]) and "advance_on_skip" (t counts skipped attempts too)."""
    ps = [p.clone().double() for p in params]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    t = step = 0
    for k, gk in enumerate(grads):
        if k in skipped:
            if fault == "advance_on_skip":
                t += 1
            continue
        idx = t + 1 if fault == "table_next" else t
        lr_now = table[min(idx, len(table) - 1)]
        step += 1
        for i, (mult, wd) in enumerate(groups):
            o, _ = adam_hp_ref(ps[i], gk[i], ms[i], vs[i], step, lr_now, mult, wd, decoupled, b1, b2, eps, bounds=False,
                               hyper32=False, fault=fault if fault in ("decay_on_grad_decoupled", "decoupled_base_lr",
                                                                       "no_mult") else None)
            ps[i], ms[i], vs[i] = o["p"].reshape(ps[i].shape), o["m"].reshape(ps[i].shape), o["v"].reshape(ps[i].shape)
        t += 1
    return ps


def torch_trajectory(params, grads, table, groups, decoupled, skipped=(), b1=0.9, b2=0.999, eps=1e-8):
    """The same run on torch.optim.Adam(weight_decay=) / torch.optim.AdamW: one torch group per group, its lr set from the table
    before every applied step, the position advanced behind `if not skipped`."""
    ps = [torch.nn.Parameter(p.clone().double()) for p in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([{"params": [p], "lr": 0.0, "weight_decay": wd} for p, (_, wd) in zip(ps, groups)], lr=0.0, betas=(b1, b2),
              eps=eps, foreach=False)
    t = 0
    for k, gk in enumerate(grads):
        if k in skipped:
            continue
        for grp, (mult, _) in zip(opt.param_groups, groups):
            grp["lr"] = table[min(t, len(table) - 1)] * mult
        for p, g in zip(ps, gk):
            p.grad = g.clone().double()
        opt.step()
        t += 1
    return [p.detach().clone() for p in ps]
