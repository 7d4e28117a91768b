"""Learning-rate tables and parameter groups for TrainStep.  Pure host code: nothing here touches a device.

A schedule is a table of floats: table[t] is the rate of the (t+1)-th applied optimiser step, and past its end the table holds
its last entry.  TrainStep uploads the table once; c2s_lr_advance reads it at a device position, so the rate moves under hipGraph
replay.
"""
from __future__ import annotations

import hashlib
import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch


def warmup_cosine(base_lr: float, warmup_steps: int, total_steps: int, min_lr: float = 0.0) -> List[float]:
    """Linear warm-up base_lr * (t + 1) / warmup_steps over the first `warmup_steps` entries, then half a cosine from base_lr
    (at t = warmup_steps) down to min_lr (at t = total_steps - 1)."""
    if total_steps < 1 or warmup_steps < 0 or warmup_steps > total_steps:
        raise ValueError(f"warmup_cosine: warmup_steps {warmup_steps}, total_steps {total_steps}")
    return [base_lr * warmup_cosine_factor(t, warmup_steps, total_steps, min_lr / base_lr if base_lr else 0.0)
            for t in range(total_steps)]


def warmup_cosine_factor(t: int, warmup_steps: int, total_steps: int, min_factor: float = 0.0) -> float:
    """The factor on base_lr at step t (the lambda of a torch LambdaLR with the same schedule)."""
    if t < warmup_steps:
        return (t + 1) / warmup_steps
    span = max(total_steps - 1 - warmup_steps, 1)
    x = min(t - warmup_steps, span) / span
    return min_factor + (1.0 - min_factor) * 0.5 * (1.0 + math.cos(math.pi * x))


def from_torch(factory: Callable, base_lr: float, steps: int) -> List[float]:
    """The rates of a torch.optim.lr_scheduler: `factory(optimizer)` builds it on a throw-away CPU optimiser at `base_lr`, and
    param_groups[0]["lr"] is recorded before each of `steps` optimizer.step() / scheduler.step() pairs."""
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)
    sched = factory(opt)
    table = []
    for _ in range(steps):
        table.append(float(opt.param_groups[0]["lr"]))
        opt.step()
        sched.step()
    return table


def no_decay_names(model) -> List[str]:
    """Names of the parameters with ndim <= 1 (norm gains, biases): the usual {"params": ..., "weight_decay": 0} group."""
    return [n for n, p in model.named_parameters() if p.ndim <= 1]


def schedule_table(lr: float, lr_schedule=None, schedule_steps: Optional[int] = None) -> List[float]:
    """The table TrainStep uploads: [lr] for None, the sequence itself, or f(t) for t in range(schedule_steps).  ValueError for
    an empty table or an entry that is not finite and >= 0."""
    if lr_schedule is None:
        table = [float(lr)]
    elif callable(lr_schedule):
        if schedule_steps is None or int(schedule_steps) < 1:
            raise ValueError("TrainStep: a callable lr_schedule needs schedule_steps >= 1")
        table = [float(lr_schedule(t)) for t in range(int(schedule_steps))]
    else:
        table = [float(v) for v in lr_schedule]
        if schedule_steps is not None and int(schedule_steps) != len(table):
            raise ValueError(f"TrainStep: lr_schedule has {len(table)} entries, schedule_steps says {schedule_steps}")
    if not table:
        raise ValueError("TrainStep: lr_schedule is empty")
    for t, v in enumerate(table):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"TrainStep: lr_schedule[{t}] = {v!r}, a finite rate >= 0 is needed")
    return table


def table_at(table: Sequence[float], t: int) -> float:
    """The entry step t uses: the last one past the end."""
    return table[min(max(int(t), 0), len(table) - 1)]


def table_digest(table: Sequence[float]) -> str:
    """sha256 of the table's float32 bytes (what the device holds)."""
    return hashlib.sha256(np.asarray(table, dtype=np.float32).tobytes()).hexdigest()


Selector = Union[str, Sequence[str], Callable[[str], bool]]


def _matches(sel: Selector, name: str) -> bool:
    if callable(sel):
        return bool(sel(name))
    if isinstance(sel, str):
        sel = [sel]
    return any(name == s or name.startswith(s) for s in sel)


def resolve_param_groups(names: Sequence[str], param_groups: Optional[Sequence[Dict]] = None,
                         weight_decay: float = 0.0) -> List[Tuple[float, float]]:
    """(lr multiplier, weight decay) of every parameter in `names`.  A group is {"params": a name prefix | a list of names or
    prefixes | a predicate on the name, "lr_mult": 1.0, "weight_decay": the global one}; unmatched parameters take
    (1, weight_decay).  ValueError for a group that matches nothing, a parameter matched by two groups, and a negative or
    non-finite multiplier or decay."""
    def checked(what: str, v) -> float:
        v = float(v)
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError(f"TrainStep: {what} = {v!r}, a finite value >= 0 is needed")
        return v

    wd0 = checked("weight_decay", weight_decay)
    out: List[Tuple[float, float]] = [(1.0, wd0)] * len(names)
    owner: Dict[int, int] = {}
    for gi, grp in enumerate(param_groups or []):
        if not isinstance(grp, dict) or "params" not in grp:
            raise ValueError(f"TrainStep: param_groups[{gi}] must be a dict with a 'params' entry")
        unknown = set(grp) - {"params", "lr_mult", "weight_decay"}
        if unknown:
            raise ValueError(f"TrainStep: param_groups[{gi}] has unknown keys {sorted(unknown)}")
        mult = checked(f"param_groups[{gi}]['lr_mult']", grp.get("lr_mult", 1.0))
        wd = checked(f"param_groups[{gi}]['weight_decay']", grp.get("weight_decay", wd0))
        hit = [i for i, n in enumerate(names) if _matches(grp["params"], n)]
        if not hit:
            raise ValueError(f"TrainStep: param_groups[{gi}] ({grp['params']!r}) matches no parameter")
        for i in hit:
            if i in owner:
                raise ValueError(f"TrainStep: parameter {names[i]!r} is matched by param_groups[{owner[i]}] and param_groups[{gi}]")
            owner[i] = gi
            out[i] = (mult, wd)
    return out
