"""Launch trace of engine.conv2d / engine.conv_transpose2d (+ tape.backward()) recorded without a GPU.

The engine reaches the library only through `engine.lib()` and the stream through `engine._stream()`.  Here `engine.lib` is
a stand-in that forwards the host-only exports (sizes, `*_supported` predicates) to the real library and records every other
call instead of launching it; the operands are CPU tensors that nothing reads.  A record holds the entry point, the bytes of
a descriptor, every number, the taps, and for each pointer the role of the tensor it points into (`src0`, `w+<float
offset>`, `bias`, `gout`, `gin0`, `valid`, `packed:<key>`, `slabs`, ...), never the address itself.

tests/golden/conv_launch_trace.json holds, per case of GRID and per switch setting, the sequence of entry points and the
SHA-256 of the full trace as the code recorded them before the convolution dispatch moved into engine.conv_plan (the commit
is named in the file).  `python tests/conv_trace.py OUT.json COMMIT` writes such a file from the checkout it runs in; only
names of the engine that existed then are used.  tests/test_conv_plan.py replays the grid and requires equality.
"""
import ctypes as C
import hashlib
import json
import os
import sys
from contextlib import contextmanager

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from crop2seg_amd import _lib  # noqa: E402
from crop2seg_amd import engine as E  # noqa: E402
from test_conv_paths_gpu import ROWS, TRANSPOSE_SHAPES  # noqa: E402

HOST_ONLY = ("_supported", "_floats", "_elems", "_bytes", "_blocks")
SWITCHES = {
    "default": {},
    "WINOGRAD=0": {"WINOGRAD": False},
    "WINO16=0": {"WINO16": False},
    "S2WINO=0": {"S2WINO": False},
    "bf16x3": {"CONV_MODE": "bf16x3"},
}
DEFAULTS = {"WINOGRAD": True, "WINO16": True, "S2WINO": True, "CONV_MODE": "f32", "REDUCE_BATCH": False, "PROFILE": None,
            "SIDE_WGRAD": False}
SAME = "same as default"


class RecordingLib:
    """engine.lib() stand-in: host-only exports run, every other call is appended to `calls` and answers 0."""

    def __init__(self):
        self.real = _lib.lib()
        self.calls = []

    def __getattr__(self, name):
        if name.endswith(HOST_ONLY) or name in ("c2s_device_cus", "c2s_last_error"):
            return getattr(self.real, name)
        argtypes = _lib.SIGNATURES[name][1]

        def record(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            rec = [name]
            for a, t in zip(args, argtypes):
                if t is C.c_void_p:
                    rec.append(("ptr", a))                       # resolved to a role once the case has run
                elif t is C.POINTER(C.c_int):
                    rec.append(("taps", list(a)))
                elif isinstance(t, type) and issubclass(t, C._Pointer):
                    rec.append(("desc", bytes(a._obj).hex()))    # C.byref(descriptor)
                else:
                    rec.append(("num", a))
            self.calls.append(rec)
            return 0
        return record


@contextmanager
def recording(switches):
    """Engine with the stand-in library, stream 0, no side stream and the given convolution switches."""
    old = {n: getattr(E, n) for n in ["lib", "_stream"] + list(DEFAULTS)}
    rec = RecordingLib()
    try:
        E.lib, E._stream = (lambda: rec), (lambda: 0)
        for n, v in {**DEFAULTS, **switches}.items():
            setattr(E, n, v)
        yield rec
    finally:
        for n, v in old.items():
            setattr(E, n, v)


def _resolve(calls, roles):
    """Pointers -> roles.  `roles`: label -> tensor (all alive, so their address ranges are disjoint)."""
    spans = [(t.data_ptr(), t.data_ptr() + max(t.numel(), 1) * t.element_size(), label) for label, t in roles.items()]

    def role(p):
        if p is None or p == 0:
            return None
        for lo, hi, label in spans:
            if lo <= p < hi:
                return label if p == lo else f"{label}+{(p - lo) // 4}"
        raise AssertionError(f"pointer into no known tensor (roles {sorted(roles)})")

    return [[c[0]] + [[k, role(v)] if k == "ptr" else [k, v] for k, v in c[1:]] for c in calls]


def _roles(ctx, named):
    roles = dict(named)
    for key, t in ctx._packed.items():
        if isinstance(t, tuple):                                 # the bf16x3 pair
            roles[f"packed:{key}:hi"], roles[f"packed:{key}:lo"] = t
        else:
            roles[f"packed:{key}"] = t
    for name, t in ctx.ws.bufs.items():
        roles["slabs" if name.startswith("wgrad_slabs") else f"ws:{name}"] = t
    for name, t in ctx.g.items():
        roles[f"g{name}"] = t
    return roles


def _ctx(params, trainable):
    g = {k: torch.empty_like(v) for k, v in params.items()}
    ctx = E.Ctx(params, {}, g, E.Workspace(torch.device("cpu")), True, E.Tape(), trainable=trainable)
    ctx.cus = 256                                                # as on an MI355X, whatever this machine has
    return ctx


def trace_conv2d(case, switches):
    N, chans, Cout, H, W, K, S, pad = (case[k] for k in ("N", "chans", "Cout", "H", "W", "K", "S", "pad"))
    pm = _lib.PAD_REFLECT if case["mode"] == "reflect" else _lib.PAD_ZEROS
    Ho, Wo = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    params = {"w": torch.empty(Cout, sum(chans), K, K)}
    if case["bias"]:
        params["b"] = torch.empty(Cout)
    srcs = [torch.empty(N, c, H, W) for c in chans]
    valid = torch.empty(N, dtype=torch.int32)
    gout = torch.empty(N, Cout, Ho, Wo)
    with recording(switches) as rec:
        ctx = _ctx(params, ["b"] if case["frozen"] else None)
        named = {"w": params["w"], "valid": valid, "gout": gout}
        if case["bias"]:
            named["bias"] = params["b"]
        for si, (s, acc) in enumerate(zip(srcs, case["acc"])):
            named[f"src{si}"] = s
            if acc:
                ctx.tape.grads[s.data_ptr()] = torch.empty_like(s)
            if case["frozen"]:
                ctx._needs.add(s.data_ptr())                     # the sources still need their gradient
        out = E.conv2d(ctx, srcs, "w", "b" if case["bias"] else None, K, S, pad, pm, valid,
                       need_input_grad=case["input_grad"])
        named["out"] = out
        if ctx.tape.ops:
            ctx.tape.grads[out.data_ptr()] = gout
            ctx.tape.backward()
        for si, s in enumerate(srcs):
            if s.data_ptr() in ctx.tape.grads:
                named[f"gin{si}"] = ctx.tape.grads[s.data_ptr()]
        return _resolve(rec.calls, _roles(ctx, named))


def trace_transpose(case, switches):
    N, Cin, Cout, H, W, K, pad = (case[k] for k in ("N", "Cin", "Cout", "H", "W", "K", "pad"))
    params = {"w": torch.empty(Cin, Cout, K, K), "b": torch.empty(Cout)}
    x = torch.empty(N, Cin, H, W)
    gout = torch.empty(N, Cout, 2 * H, 2 * W)
    with recording(switches) as rec:
        ctx = _ctx(params, None)
        if case["acc"]:
            ctx.tape.grads[x.data_ptr()] = torch.empty_like(x)
        out = E.conv_transpose2d(ctx, x, "w", "b", K, pad)
        ctx.tape.grads[out.data_ptr()] = gout
        ctx.tape.backward()
        named = {"w": params["w"], "bias": params["b"], "src0": x, "gout": gout, "out": out,
                 "gin0": ctx.tape.grads[x.data_ptr()]}
        return _resolve(rec.calls, _roles(ctx, named))


def _grid():
    geoms = [(f"row:{r.id}", r.N, r.chans, r.Cout, r.H, r.W, r.K, r.S, 0 if r.K == 1 else 1, r.acc) for r in ROWS]
    for cin in (4, 10):                                          # first layers
        for hw in ((128, 128), (20, 36)):
            geoms.append((f"first:{cin}:{hw[0]}x{hw[1]}", 3, (cin,), 64, *hw, 3, 1, 1, (0,)))
    geoms.append(("1x1", 3, (64,), 64, 32, 32, 1, 1, 0, (0,)))
    for K, pad in ((4, 1), (2, 0), (6, 2)):                      # stride-2 down convolutions, wide and narrow planes
        for hw in (128, 32):
            for acc in (0, 1):
                geoms.append((f"s2:k{K}:{hw}:acc{acc}", 3, (64,), 64, hw, hw, K, 2, pad, (acc,)))
    variants = {"base": {}, "nobias": {"bias": False}, "noinputgrad": {"input_grad": False}, "frozen": {"frozen": True}}
    cases = []
    for gid, N, chans, Cout, H, W, K, S, pad, acc in geoms:
        for mode in ("zeros", "reflect"):
            for vid, v in variants.items():
                cases.append({"id": f"conv2d:{gid}:{mode}:{vid}", "op": "conv2d", "N": N, "chans": list(chans), "Cout": Cout,
                              "H": H, "W": W, "K": K, "S": S, "pad": pad, "mode": mode, "acc": list(acc),
                              **{"bias": True, "input_grad": True, "frozen": False, **v}})
    for N, Cin, Cout, H, W in TRANSPOSE_SHAPES:
        for K, pad in ((4, 1), (2, 0), (6, 2)):
            for acc in (0, 1):
                cases.append({"id": f"transpose:{N}x{Cin}x{Cout}x{H}x{W}:k{K}:acc{acc}", "op": "transpose", "N": N, "Cin": Cin,
                              "Cout": Cout, "H": H, "W": W, "K": K, "pad": pad, "acc": acc})
    return cases


GRID = _grid()


def summary(case, switches):
    """What the golden file keeps of one trace: the entry points in clear text and the SHA-256 of everything."""
    trace = (trace_conv2d if case["op"] == "conv2d" else trace_transpose)(case, switches)
    digest = hashlib.sha256(json.dumps(trace, sort_keys=True).encode()).hexdigest()
    return {"calls": " ".join(c[0][len("c2s_"):] for c in trace), "sha256": digest}


def record_case(case):
    """Switch setting -> summary; a setting whose trace is the default one says so instead of repeating it."""
    out = {sw: summary(case, sv) for sw, sv in SWITCHES.items()}
    return {sw: SAME if sw != "default" and s == out["default"] else s for sw, s in out.items()}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({"recorded_at_commit": sys.argv[2], "cases": {c["id"]: record_case(c) for c in GRID}}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
