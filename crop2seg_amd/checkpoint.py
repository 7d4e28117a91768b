"""Checkpoints of a TrainStep: the host side of csrc/snapshot.hip (checkpoints).

Pure host code, testable without a GPU: the blob layout (`plan_layout`, `blob_header`, `word_sums`), the two conversions
between the flat training state and the reference's file format (`flat_to_torch`, `torch_to_flat`), and `Snapshot`, the handle
`TrainStep.snapshot()` returns.  The launches are in engine.py, the orchestration in learning/utils.py (TrainStep).

File format: the reference's `{"epoch", "best_mIoU", "state_dict", "optimizer"}` (train.py:531-541) plus `"crop2seg_amd"`:
`state_dict` is exactly model.state_dict(), `optimizer` a torch.optim.Adam state dict indexed in model.parameters() order.
"""
from __future__ import annotations

import struct
import warnings
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import (SNAPSHOT_HEADER_BYTES, SNAPSHOT_MAGIC, SNAPSHOT_SPAN_BYTES, SNAPSHOT_VERSION)

Tensor = torch.Tensor
LAYOUT_VERSION = 1
EXTRA_KEY = "crop2seg_amd"
_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- blob layout
def plan_layout(region_bytes: Sequence[int]) -> Tuple[List[int], int, List[int]]:
    """(payload offset of every region, payload bytes, first virtual block of every region).  A region is any multiple of 4
    bytes (zero allowed), starts on a multiple of 16 and is padded with zero words to the next one; a padded region is cut into
    spans of SNAPSHOT_SPAN_BYTES, one virtual block each."""
    offs, blocks, o, b = [], [], 0, 0
    for n in region_bytes:
        n = int(n)
        if n < 0 or n % 4:
            raise ValueError(f"plan_layout: a region of {n} bytes, a non-negative multiple of 4 is needed")
        offs.append(o)
        blocks.append(b)
        padded = (n + 15) // 16 * 16
        o += padded
        b += (padded + SNAPSHOT_SPAN_BYTES - 1) // SNAPSHOT_SPAN_BYTES
    return offs, o, blocks


def word_sums(words: np.ndarray, first_index: int = 0) -> Tuple[int, int]:
    """(s1, s2) of 32-bit words w_i that sit at payload indices first_index + i: s1 = sum w_i, s2 = sum (index + 1) w_i, both
    mod 2^64 (numpy's uint64 arithmetic wraps)."""
    w = np.ascontiguousarray(words).view(np.uint32).astype(np.uint64)
    if w.size == 0:
        return 0, 0
    with np.errstate(over="ignore"):
        idx = np.arange(1, w.size + 1, dtype=np.uint64) + np.uint64(first_index)
        return int(w.sum(dtype=np.uint64)), int((idx * w).sum(dtype=np.uint64))


def compose_sums(parts: Sequence[Tuple[int, int, int]]) -> Tuple[int, int]:
    """Sums of a payload from its regions' own sums: parts = (payload offset in bytes, s1, s2 with indices counted from the
    region's start).  Zero padding adds nothing."""
    s1 = s2 = 0
    for off, a, b in parts:
        s1 = (s1 + a) & _M64
        s2 = (s2 + b + (off // 4) * a) & _M64
    return s1, s2


def blob_header(nregions: int, payload_bytes: int, s1: int, s2: int) -> bytes:
    return struct.pack("<IIIIQQQ24x", SNAPSHOT_MAGIC, SNAPSHOT_VERSION, nregions, 0, payload_bytes, s1 & _M64, s2 & _M64)


def parse_header(raw: bytes) -> Dict[str, int]:
    magic, version, nregions, _, payload, s1, s2 = struct.unpack("<IIIIQQQ24x", bytes(raw[:SNAPSHOT_HEADER_BYTES]))
    return {"magic": magic, "version": version, "nregions": nregions, "payload_bytes": payload, "s1": s1, "s2": s2}


# ---------------------------------------------------------------------------------------------------------------- conversions
def adam_skeleton(nparams: int, lr: float, betas: Tuple[float, float], eps: float) -> dict:
    """state_dict() of a throw-away torch.optim.Adam over `nparams` CPU parameters: the param_groups keys of the running
    torch, none written by hand."""
    ps = [torch.nn.Parameter(torch.zeros(1)) for _ in range(nparams)]
    return torch.optim.Adam(ps, lr=lr, betas=tuple(betas), eps=eps).state_dict()


def flat_to_torch(keys: Sequence[str], names: Sequence[str], shapes: Sequence[Sequence[int]], offsets: Sequence[int],
                  flat_param: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, param_steps: Sequence[int],
                  buffers: Dict[str, Tensor], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                  eps: float = 1e-8) -> dict:
    """The flat training state in torch's format.  keys: the order of model.state_dict(); names / shapes / offsets: the
    parameters in model.parameters() order with their offsets (in floats) into the three flat CPU tensors; buffers: every
    entry of `keys` that is no parameter.  A parameter whose step count is 0 gets no optimiser state, as in torch."""
    def cut(flat, i):
        n = 1
        for s in shapes[i]:
            n *= int(s)
        return flat[offsets[i]:offsets[i] + n].reshape(tuple(shapes[i])).clone()

    index = {n: i for i, n in enumerate(names)}
    sd = OrderedDict()
    for k in keys:
        sd[k] = cut(flat_param, index[k]) if k in index else buffers[k].clone()
    opt = adam_skeleton(len(names), lr, betas, eps)
    for i, st in enumerate(param_steps):
        if st > 0:
            opt["state"][i] = {"step": torch.tensor(float(st)), "exp_avg": cut(exp_avg, i), "exp_avg_sq": cut(exp_avg_sq, i)}
    return {"state_dict": sd, "optimizer": opt}


def torch_to_flat(state: dict, names: Sequence[str], shapes: Sequence[Sequence[int]], offsets: Sequence[int], total: int):
    """The inverse: (flat_param, exp_avg, exp_avg_sq, param_steps, buffers) as CPU tensors, the padding between slots zero.
    Raises ValueError listing every parameter that is missing or has another shape."""
    sd, opt = state["state_dict"], state.get("optimizer")
    flats = [torch.zeros(total, dtype=torch.float32) for _ in range(3)]
    steps, diffs = [0] * len(names), []
    ostate = {} if opt is None else opt.get("state", {})
    if opt is not None:
        nopt = sum(len(g["params"]) for g in opt["param_groups"])
        if nopt != len(names):
            diffs.append(f"optimizer: {nopt} parameters, the model has {len(names)}")
    for i, (n, shp, off) in enumerate(zip(names, shapes, offsets)):
        if n not in sd:
            diffs.append(f"{n}: missing")
            continue
        if tuple(sd[n].shape) != tuple(shp):
            diffs.append(f"{n}: shape {tuple(sd[n].shape)}, the model has {tuple(shp)}")
            continue
        cnt = sd[n].numel()
        flats[0][off:off + cnt] = sd[n].detach().to(torch.float32).reshape(-1)
        st = ostate.get(i)
        if st is not None:
            if tuple(st["exp_avg"].shape) != tuple(shp):
                diffs.append(f"optimizer state {i} ({n}): shape {tuple(st['exp_avg'].shape)}, the model has {tuple(shp)}")
                continue
            steps[i] = int(st["step"])
            flats[1][off:off + cnt] = st["exp_avg"].detach().to(torch.float32).reshape(-1)
            flats[2][off:off + cnt] = st["exp_avg_sq"].detach().to(torch.float32).reshape(-1)
    if diffs:
        raise ValueError("checkpoint does not fit the model:\n  " + "\n  ".join(diffs))
    pset = set(names)
    buffers = {k: v.detach() for k, v in sd.items() if k not in pset}
    return flats[0], flats[1], flats[2], steps, buffers


def is_bit_exact(state: dict) -> bool:
    """Whether a state continues bit for bit: only with our own key (seed record, guard counters); a file with the
    reference's keys alone loads parameters, buffers and moments, and its dropout sequence starts fresh."""
    return isinstance(state.get(EXTRA_KEY), dict) and state[EXTRA_KEY].get("layout_version") == LAYOUT_VERSION


# ---------------------------------------------------------------------------------------------------------------- Snapshot
class Snapshot:
    """The training state at one point of the stream: a pinned host blob that a side stream fills behind an event, the
    layout it was gathered with and the host-side scalars read when snapshot() was called.  Made by TrainStep.snapshot()."""

    def __init__(self, host_blob: Tensor, done, regions: List[Tuple[str, int, int]], meta: dict):
        self.host_blob, self._done = host_blob, done
        self.regions = regions              # (name, bytes, payload offset)
        self.meta = meta
        self._state: Optional[dict] = None

    def wait(self) -> "Snapshot":
        """Wait for the copy to the host (the only host synchronisation of a snapshot)."""
        if self._done is not None:
            self._done.synchronize()
            self._done = None
        return self

    def region(self, name: str) -> np.ndarray:
        """A region's bytes as uint32 words (a view of the host blob)."""
        self.wait()
        for n, nb, off in self.regions:
            if n == name:
                a = SNAPSHOT_HEADER_BYTES + off
                return self.host_blob.numpy()[a:a + nb].view(np.uint32)
        raise KeyError(name)

    def _tensor(self, name: str, dtype) -> Tensor:
        return torch.from_numpy(self.region(name).view(np.int32).copy()).view(dtype)

    def state_dict(self) -> dict:
        """CPU tensors in the file format (module docstring).  The step counts and the skip count are the device's, out of
        the blob.  Raises RuntimeError when the blob's header does not agree with its payload."""
        if self._state is not None:
            return self._state
        self.wait()
        m = self.meta
        raw = self.host_blob.numpy()
        h = parse_header(raw)
        parts, sums = [], []
        for n, nb, off in self.regions:
            a, b = word_sums(self.region(n))
            parts.append((off, a, b))
            sums.append([n, nb, a, b])
        s1, s2 = compose_sums(parts)
        if (h["magic"], h["version"], h["nregions"], h["payload_bytes"]) != (SNAPSHOT_MAGIC, SNAPSHOT_VERSION, len(self.regions),
                                                                            raw.size - SNAPSHOT_HEADER_BYTES) \
                or (h["s1"], h["s2"]) != (s1, s2):
            raise RuntimeError(f"Snapshot: the blob's header {h} does not agree with its payload (sums {s1}, {s2})")
        have = {n for n, _, _ in self.regions}
        param_steps, skipped, step_count = list(m["param_steps"]), 0, m["step_count"]
        if m["guard"] is not None:
            param_steps = [int(v) for v in self._tensor("slot_steps_dev", torch.int32)]
            skipped = int(self._tensor("_skip_dev", torch.int32)[0])
            step_count = m["attempts"] - skipped
        optim, lr = m.get("optim"), m["lr"]
        if optim is not None:
            # schedule path: the step counts and the schedule block are the device's own bytes at the snapshot's place in the
            # stream; the optimizer entry's lr is the rate at that position
            param_steps = [int(v) for v in self._tensor("slot_steps_dev", torch.int32)]
            words = self._tensor("sched_dev", torch.int32)
            t, scale = int(words[0]), float(words.view(torch.float32)[1])
            table = optim["table"]
            lr = float(np.float32(np.float64(np.float32(table[min(max(t, 0), len(table) - 1)])) * np.float64(scale)))
        buffers: Dict[str, Tensor] = {}
        if "flat_buf" in have:
            fb, o = self._tensor("flat_buf", torch.float32), 0
            for k, shp in m["flat_buf_views"]:
                n = int(np.prod(shp, dtype=np.int64))
                buffers[k] = fb[o:o + n].reshape(tuple(shp)).clone()
                o += (n + 3) // 4 * 4
        for k, shp, dt in m["buffers"]:
            buffers[k] = self._tensor("buffer:" + k, dt).reshape(tuple(shp))
        state = flat_to_torch([k for k in m["keys"]], m["names"], m["shapes"], m["offsets"],
                              self._tensor("flat_param", torch.float32), self._tensor("exp_avg", torch.float32),
                              self._tensor("exp_avg_sq", torch.float32), param_steps, buffers, lr, m["betas"], m["eps"])
        if optim is not None:
            for grp in state["optimizer"]["param_groups"]:
                grp["weight_decay"] = optim["weight_decay"]
        capture = None
        if m["capture"] is not None:
            capture = dict(m["capture"])
            capture["seed_dev"] = int(self._tensor("seed_dev", torch.int64)[0])
            if "step_dev" in have:
                capture["step_dev"] = [int(v) for v in self._tensor("step_dev", torch.int32)]
        state[EXTRA_KEY] = {
            "layout_version": LAYOUT_VERSION, "s1": s1, "s2": s2, "regions": sums,
            "guard": None if m["guard"] is None else dict(m["guard"], attempts=m["attempts"], skipped=skipped),
            "step_count": step_count, "param_steps": param_steps, "seed_root": m["seed_root"], "seed_calls": m["seed_calls"],
            "rank": m["rank"], "capture": capture, "trainable": dict(m["trainable"]),
            "hyper": {"lr": m["lr"], "betas": list(m["betas"]), "eps": m["eps"]},
            "extra_buffers": {k: buffers[k] for k in buffers if k not in state["state_dict"]},
        }
        if optim is not None:               # only then: a state of a step without the schedule path keeps its bytes
            state[EXTRA_KEY]["optim"] = {
                "table_len": optim["table_len"], "table_digest": optim["table_digest"], "groups": dict(optim["groups"]),
                "decoupled": optim["decoupled"], "weight_decay": optim["weight_decay"], "sched_words": [int(w) for w in words]}
        self._state = state
        return state

    def save(self, path, epoch: Optional[int] = None, best_mIoU: Optional[float] = None) -> None:
        """wait(), then torch.save of state_dict() with the reference's `epoch` / `best_mIoU` keys when given."""
        state = dict(self.state_dict())
        if epoch is not None:
            state["epoch"] = epoch
        if best_mIoU is not None:
            state["best_mIoU"] = best_mIoU
        torch.save(state, path)


def warn_not_bit_exact() -> None:
    warnings.warn("crop2seg_amd: the checkpoint has only the reference's keys: parameters, buffers, moments and step counts are "
                  "loaded, the dropout sequence starts fresh -- the continuation is not bit-exact")
