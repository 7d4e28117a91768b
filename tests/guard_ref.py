"""float64 reference of the guarded optimiser step (csrc/guard.hip; TrainStep(max_grad_norm=..., skip_nonfinite=...)):

    total = grad_scale * sqrt(sum of g^2 over the trainable slots)           (fp64; the padding and frozen slots are not read)
    coef  = min(1, max_grad_norm / (total + 1e-6))   (torch.nn.utils.clip_grad_norm_, norm_type 2; 1 without a threshold)
    ok    = not skip_nonfinite or isfinite(sum)
    ok:   every trainable slot takes tail_ref.adam_ref with its own step count + 1 and grad_scale * coef
    else: nothing changes (torch.optim.Adam when step() is not called), the skip counter advances

The kernels round grad_scale * coef once to float32 and hand that to Adam; `scale32` feeds that very number (read back from the
status block) to the reference, so that the Adam bars of tests/tail_ref.py hold unchanged.
"""
import math

import numpy as np
import torch

import tail_ref as R


def sumsq_ref(g, slots, flags):
    """Sum of squares of the trainable slots in float64 (numpy), and the number of elements it covers."""
    g = np.asarray(g, dtype=np.float32)
    total, n = 0.0, 0
    with np.errstate(over="ignore", invalid="ignore"):
        for (off, ln), f in zip(slots, flags):
            if f:
                x = g[off:off + ln].astype(np.float64)
                total += float(np.sum(x * x))
                n += ln
    return total, n


def decide_ref(sumsq, max_grad_norm, grad_scale, skip_nonfinite):
    """(ok, norm, coef, scale) in float64; max_grad_norm and grad_scale are taken as the float32 values the kernel receives."""
    gs = float(np.float32(grad_scale))
    ok = (not skip_nonfinite) or math.isfinite(sumsq)
    norm = gs * math.sqrt(sumsq) if sumsq >= 0 else float("nan")
    coef = 1.0
    if max_grad_norm is not None:
        c = float(np.float32(max_grad_norm)) / (norm + 1e-6)
        coef = c if c < 1.0 else 1.0
    return ok, norm, coef, gs * coef


def guard_ref(p, g, m, v, steps, slots, flags, max_grad_norm=None, skip_nonfinite=False, grad_scale=1.0, lr=1e-3, b1=0.9,
              b2=0.999, eps=1e-8, scale32=None, bounds=True):
    """One guarded step on flat tensors.  slots: (offset, length) per slot; flags: trainable or not; steps: the Adam step count
    of every slot BEFORE this step.  Returns a dict: p, m, v (float64 flat tensors: new values inside trainable slots, the old
    ones elsewhere), steps (after), ok, norm, coef, scale, skipped (0 / 1) and per_slot = {slot index: (out, A)} of
    tail_ref.adam_ref for the slots that stepped."""
    p64, m64, v64 = (torch.as_tensor(x).detach().double().reshape(-1).clone() for x in (p, m, v))
    g32 = torch.as_tensor(g).detach().float().reshape(-1)
    ss, _ = sumsq_ref(g32.numpy(), slots, flags)
    ok, norm, coef, scale = decide_ref(ss, max_grad_norm, grad_scale, skip_nonfinite)
    out = {"p": p64, "m": m64, "v": v64, "steps": list(steps), "ok": ok, "norm": norm, "coef": coef, "scale": scale,
           "sumsq": ss, "skipped": 0 if ok else 1, "per_slot": {}}
    if not ok:
        return out
    use = scale if scale32 is None else float(scale32)
    p0, m0, v0 = p64.clone(), m64.clone(), v64.clone()
    for i, ((off, ln), f) in enumerate(zip(slots, flags)):
        if not f:
            continue
        out["steps"][i] = steps[i] + 1
        s = slice(off, off + ln)
        o, A = R.adam_ref(p0[s], g32[s], m0[s], v0[s], steps[i] + 1, lr=lr, b1=b1, b2=b2, eps=eps, grad_scale=use, bounds=bounds)
        p64[s], m64[s], v64[s] = o["p"], o["m"], o["v"]
        out["per_slot"][i] = (o, A)
    return out
