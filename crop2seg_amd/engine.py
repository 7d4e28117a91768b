"""Host-side execution engine: thin op wrappers over the C ABI (libc2s_hip.so) and an explicit backward tape.

PyTorch is used for device memory (torch.empty on the current HIP device), the current stream and
nn.Parameter storage only -- every activation-sized computation below is a hand-written HIP kernel.
The tape is a plain list of closures recorded during the forward pass and replayed in reverse: no
tracing, no autograd graph, stream-ordered launches only (hipGraph-capturable).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import AggDesc, C2SError, ConvDesc, LtaeDesc, NormDesc, WgradDesc, check, lib

Tensor = torch.Tensor


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


import os as _os

_SIDE = None
SIDE_WGRAD = _os.environ.get("C2S_WGRAD_STREAM", "1") != "0"
SIDE_BATCH = int(_os.environ.get("C2S_WGRAD_BATCH", "8"))
SIDE_FLUSH_POSITIONS = int(_os.environ.get("C2S_WGRAD_FLUSH_POSITIONS", str(1 << 22)))
# While a hipGraph is being captured the fork / join events become cross-stream edges of the graph.  Measured (round 3,
# U-TAE B=4 T=32): the captured two-stream step replays at 17.1 ms against 12.65 ms for the single-stream capture and
# 12.25 ms for eager two-stream launches -- the graph executor serialises around the cross-stream edges -- so a capture stays
# on one stream unless C2S_GRAPH_SIDE=1.
GRAPH_SIDE = _os.environ.get("C2S_GRAPH_SIDE", "0") != "0"
# The aggregator's input gradient up(attn) * d skip as a pending term of the tape: temporal_aggregate's backward stores the
# interpolated weights once and the 4x4 stride-2 data gradient that follows adds the products in its epilogue
# (c2s_conv4x4s2_dgrad_winograd_skip) instead of reading them back from the gradient buffer.  C2S_AGG_SKIP_TERM=0: the
# aggregator writes the products and the data gradient accumulates (A/B runs; bit-identical results).
AGG_SKIP_TERM = _os.environ.get("C2S_AGG_SKIP_TERM", "1") != "0"


# Backward launch log: None (default) or a list to which every backward launch appends (op, name, kind), kind "dgrad" (the
# data gradient into an input), "wgrad" (a weight gradient) or "params" (a fused parameter-gradient launch).  Tests set it to
# show which launches a frozen parameter pruned.
BACKWARD_LOG: Optional[list] = None


def _log(op: str, name: str, kind: str) -> None:
    if BACKWARD_LOG is not None:
        BACKWARD_LOG.append((op, name, kind))


def _side_ok() -> bool:
    """Parameter-gradient launches go to the side stream (eager always; under capture when GRAPH_SIDE)."""
    return SIDE_WGRAD and (GRAPH_SIDE or not torch.cuda.is_current_stream_capturing())


def _side_stream():
    global _SIDE
    if _SIDE is None:
        _SIDE = torch.cuda.Stream()
    return _SIDE


class PackRecord(NamedTuple):
    """One weight pack of a step, as c2s_pack_job_fill takes it (the field order is the positional record's of earlier
    versions: callers that index it keep working)."""
    src_ptr: int
    cin: int
    cout: int
    coutP: int
    ntaps: int
    so: int
    sc: int
    kind: int
    taps: Tuple[int, ...]
    nfloats: int


# pack kind -> (output-channel padding, packed-size export, pack export): 0 wpk[tap][cin][coutP]; 1 / 2 Winograd U of the
# 4-wave / 8-wave 3x3 kernels; 3 / 4 F(2x2,2x2) U of the 4x4 stride-2 forward / data gradient (the layouts: pack.hip)
PACK_KINDS = {0: (32, None, "c2s_pack_weights"),
              1: (64, "c2s_winograd_packed_floats", "c2s_pack_weights_winograd"),
              2: (64, "c2s_winograd16_packed_floats", "c2s_pack_weights_winograd16"),
              3: (64, "c2s_s2wino_packed_floats", "c2s_pack_weights_s2wino"),
              4: (64, "c2s_s2dgrad_packed_floats", "c2s_pack_weights_s2dgrad")}


def _tap_array(offs: Sequence[int]):
    return (C.c_int * len(offs))(*offs)


class Workspace:
    """Named scratch buffers, grown on demand and reused across calls (never freed inside a step)."""

    def __init__(self, device):
        self.device = device
        if getattr(device, "type", None) == "cuda":
            idx = device.index if device.index is not None else torch.cuda.current_device()
            with torch.cuda.device(idx):
                _lib.init_device(idx)              # one-time per device, before any launch or hipGraph capture
        self.bufs: Dict[str, Tensor] = {}
        # weight-pack plan: the jobs recorded during one step become a device table that later steps run in one launch
        self.pack_record: Dict[Tuple, PackRecord] = {}
        self.pack_plan: Optional[dict] = None
        self.reduce_jobs: List[Tuple] = []          # slice sums of the weight gradients recorded during this backward pass
        self.reduce_post: List[Tuple] = []          # accumulating slice sums (their slab tensors held): launched after the batch
        self.reduce_plan: Optional[dict] = None     # their one-launch table (built once, reused while the jobs stay the same)

    def finalize_pack_plan(self) -> None:
        """Turn the packs recorded during the step that just ran into a one-launch plan (host -> device table copy:
        call outside hipGraph capture; TrainStep does it at the end of every eager forward/backward)."""
        if self.pack_plan is not None or not self.pack_record:
            return
        L_ = lib()
        rec_bytes = L_.c2s_pack_job_bytes()
        jobs = list(self.pack_record.items())
        table = torch.zeros(len(jobs) * rec_bytes, dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else \
            torch.zeros(len(jobs) * rec_bytes, dtype=torch.uint8)
        outs, block = {}, 0
        for i, (key, r) in enumerate(jobs):
            out = torch.empty(r.nfloats, device=self.device, dtype=torch.float32)
            check(L_.c2s_pack_job_fill(table.data_ptr() + i * rec_bytes, r.src_ptr, out.data_ptr(), r.cin, r.cout, r.coutP,
                                       r.ntaps, r.so, r.sc, r.kind, _tap_array(r.taps), block), "pack_job_fill")
            block += L_.c2s_pack_job_blocks(r.cin, r.coutP, r.ntaps, r.kind)
            outs[key] = (out, r.src_ptr)
        self.pack_plan = {"table": table.to(self.device), "njobs": len(jobs), "blocks": block, "outs": outs}
        self.pack_record = {}

    def run_reduce_batch(self) -> None:
        """Sum the split-K slabs of every weight gradient recorded during this backward pass in one launch
        (c2s_wgrad_reduce_batch).  The job table is built on the host the first time (and again if a job changed) -- outside
        hipGraph capture; under capture a matching table must exist, otherwise the sums are launched one by one.
        The accumulating sums (a weight written a second time in the tape) follow, in recording order: the batch holds the
        first, overwriting sum of the same weight, so an accumulating sum launched before it would be lost."""
        jobs, self.reduce_jobs = self.reduce_jobs, []
        post, self.reduce_post = self.reduce_post, []
        if jobs:
            self._reduce_batch(jobs, {j[0].data_ptr() for j in post})
        for (slabs, dst_ptr, so, sc, taps, d) in post:
            check(lib().c2s_wgrad_reduce(C.byref(d), slabs.data_ptr(), dst_ptr, so, sc, _tap_array(taps), 1, _stream()),
                  "wgrad_reduce")

    def _reduce_batch(self, jobs: List[Tuple], post_slabs: set) -> None:
        L_ = lib()
        key = tuple(j[:-1] for j in jobs)
        plan = self.reduce_plan
        if plan is None or plan["key"] != key:
            if torch.cuda.is_current_stream_capturing():
                import warnings
                warnings.warn("crop2seg_amd: the batched weight-gradient slice sum has no job table for this capture (the warm-up "
                              "pass ran other layers or buffers): falling back to one launch per layer inside the graph")
                for (dbytes, slabs_ptr, dst_ptr, so, sc, taps, acc, d) in jobs:
                    check(L_.c2s_wgrad_reduce(C.byref(d), slabs_ptr, dst_ptr, so, sc, _tap_array(taps), acc, _stream()), "wgrad_reduce")
                return
            rec = L_.c2s_wgrad_reduce_job_bytes()
            table = torch.zeros(len(jobs) * rec, dtype=torch.uint8).pin_memory()
            block = 0
            for i, (dbytes, slabs_ptr, dst_ptr, so, sc, taps, acc, d) in enumerate(jobs):
                check(L_.c2s_wgrad_reduce_job_fill(table.data_ptr() + i * rec, C.byref(d), slabs_ptr, dst_ptr, so, sc,
                                                   _tap_array(taps), acc, block), "wgrad_reduce_job_fill")
                block += L_.c2s_wgrad_reduce_job_blocks(C.byref(d))
            plan = self.reduce_plan = {"key": key, "table": table.to(self.device), "njobs": len(jobs), "blocks": block}
            # one slab buffer per weight lives as long as the plan (nslices * taps * CinP * CoutB floats each, ~70 MB for a U-TAE
            # step): buffers of an older plan (re-allocated gradient tensors) are dropped here
            live = {j[1] for j in jobs} | post_slabs
            for name in [k for k, b in self.bufs.items() if k.startswith("wgrad_slabs:") and b.data_ptr() not in live]:
                del self.bufs[name]
        check(L_.c2s_wgrad_reduce_batch(plan["table"].data_ptr(), plan["njobs"], plan["blocks"], _stream()), "wgrad_reduce_batch")

    def sync_area(self, nbytes: int) -> Tensor:
        """Zero-initialised area for kernels whose workgroups meet through memory (one-pass normalisation): all zero at rest
        (the kernels restore that state themselves), one area per workspace = per stream of launches.  When the area grows,
        the error word of the old one is carried over (device copy, stream-ordered)."""
        b = self.bufs.get("sync")
        if b is None or b.numel() < nbytes:
            nb = torch.zeros(max(int(nbytes), 4096), device=self.device, dtype=torch.uint8)
            if b is not None:
                nb[12:16].copy_(b[12:16])
            b = self.bufs["sync"] = nb
        return b

    def sync_error(self) -> int:
        """Error word of the sync area (host synchronisation): non-zero when a wait gave up."""
        b = self.bufs.get("sync")
        return 0 if b is None else int(b[:16].view(torch.int32)[3])

    def check_sync(self) -> None:
        """Raise if a one-pass normalisation wait gave up since the last check (host synchronisation -- call where the
        caller synchronises anyway).  The groups that gave up wrote NaN, so the step that hit it is lost; recovery: the area
        is re-zeroed and the process falls back to the two-pass normalisation kernels (`engine.ONEPASS_NORM = False`),
        which need no residency assumption.  Whether the caller may catch the error and repeat the step depends on what the
        lost step did to the optimiser state: under TrainStep(skip_nonfinite=True) the device skipped it and nothing changed;
        without that guard (or in a loop of the caller's own that ran an optimiser on the NaN gradient) the parameters, Adam
        moments and BatchNorm running statistics are NaN by now and the last checkpoint has to be restored
        (`TrainStep.load(path)`, or `TrainStep.load_state_dict(snapshot.state_dict())` for a snapshot kept in memory)."""
        if self.sync_error() == 0:
            return
        global ONEPASS_NORM
        ONEPASS_NORM = False
        torch.cuda.synchronize(self.device)
        self.bufs["sync"].zero_()
        raise RuntimeError(
            "crop2seg_amd: a one-pass normalisation wait gave up (the workgroups of a group were not co-resident: "
            "shared or masked GPU, profiler serialisation?).  The affected outputs are NaN.  The sync area has been "
            "reset and this process now uses the two-pass normalisation kernels.  Repeat the step if it was a forward pass or "
            "a TrainStep(skip_nonfinite=True) step (the device skipped the update); otherwise the NaN has reached the "
            "parameters, the Adam moments and the BatchNorm running statistics: restore the last checkpoint with "
            "TrainStep.load(path) (written by TrainStep.snapshot().save(path)).")

    def get(self, name: str, nfloats: int) -> Tensor:
        b = self.bufs.get(name)
        if b is None or b.numel() < nfloats:
            b = torch.empty(max(int(nfloats), 1), device=self.device, dtype=torch.float32)
            self.bufs[name] = b
        return b


class Tape:
    """Reverse-mode tape.  Gradients are keyed by the data pointer of the forward activation, so a tensor and
    its reshaped views (4-D frames <-> 5-D [B,T,...]) share one gradient buffer."""

    def __init__(self):
        self.ops: List[Callable[[], None]] = []
        self.grads: Dict[int, Tensor] = {}
        self.keep: List[Tensor] = []      # keeps forward tensors alive (ids stay unique)
        self.side_keep: List[Tensor] = []  # operands of kernels running on the side stream (alive until the join)
        self.side_used = False
        self.side_pending: List[Callable[[], None]] = []   # weight-gradient launches waiting for the next fork
        self.finalizers: Dict[int, Callable[[], None]] = {}   # run once after the last side-stream launch (batched slice sums)
        # data pointer of a conv2d source whose data gradient is the F(2x2,2x2) kernel -> (its descriptor, pointer of its frame
        # flags); and the terms up(attn) * d skip that temporal_aggregate left for such a source instead of writing them
        self.s2d_sources: Dict[int, Tuple[object, Optional[int]]] = {}
        self.skip_terms: Dict[int, "SkipTerm"] = {}

    def fork(self) -> "torch.cuda.Stream":
        """Side HIP stream ordered after everything issued so far on the current stream.  Weight gradients feed nothing
        until the optimizer, so they run there, next to the data-gradient chain, and fill the CUs that the small
        kernels of the chain (16x16 maps, decoder at N = B, L-TAE) leave idle; `backward()` joins the stream."""
        side = _side_stream()
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        self.side_used = True
        return side

    def record(self, fn: Callable[[], None]) -> None:
        self.ops.append(fn)

    def track(self, t: Tensor) -> Tensor:
        self.keep.append(t)
        return t

    def settle(self, key: int) -> None:
        """Write a pending skip term of the gradient buffer `key` into it: every reader but the data gradient that takes the
        term itself (take_skip_term) sees the buffer temporal_aggregate would have written (the same rounded products)."""
        term = self.skip_terms.pop(key, None)
        if term is not None:
            check(lib().c2s_agg_skip_term(C.byref(term.desc), term.a_up.data_ptr(), term.gskip.data_ptr(), _ptr(term.valid),
                                          self.grads[key].data_ptr(), _stream()), "agg_skip_term")

    def take_skip_term(self, t: Tensor) -> Optional["SkipTerm"]:
        return self.skip_terms.pop(t.data_ptr(), None)

    def grad_of(self, t: Tensor) -> Optional[Tensor]:
        self.settle(t.data_ptr())
        return self.grads.get(t.data_ptr())

    def pop_grad(self, t: Tensor) -> Optional[Tensor]:
        self.settle(t.data_ptr())
        return self.grads.pop(t.data_ptr(), None)

    def add_grad(self, t: Tensor, g: Tensor, own: bool = True) -> None:
        """Accumulate g into the gradient of t.  If t has no gradient yet, g becomes it (own=True) or is copied."""
        self.settle(t.data_ptr())
        cur = self.grads.get(t.data_ptr())
        if cur is None:
            self.grads[t.data_ptr()] = g if own else g.clone()
        else:
            check(lib().c2s_add_inplace(cur.data_ptr(), g.data_ptr(), g.numel(), _stream()), "add_inplace")

    def grad_buffer(self, t: Tensor) -> Tuple[Tensor, int]:
        """(gradient buffer of t, accumulate flag) for a kernel that adds in place: the buffer already on the tape with
        flag 1, else a fresh one nobody else holds, now on the tape, with flag 0 (the kernel overwrites it)."""
        self.settle(t.data_ptr())
        g = self.grads.get(t.data_ptr())
        if g is not None:
            return g, 1
        g = self.grads[t.data_ptr()] = torch.empty_like(t)
        return g, 0

    def defer(self, fn: Callable[[], None], keep: Sequence[Tensor]) -> None:
        """Queue a launch for the side stream; a fork is issued every SIDE_BATCH launches (each fork/join is an edge of
        the captured hipGraph, and edges are not free)."""
        self.side_pending.append(fn)
        self.side_keep.extend(keep)
        if len(self.side_pending) >= SIDE_BATCH:
            self.flush_side()

    def flush_side(self) -> None:
        if not self.side_pending:
            return
        with torch.cuda.stream(self.fork()):
            for fn in self.side_pending:
                fn()
        self.side_pending.clear()

    def backward(self) -> None:
        for fn in reversed(self.ops):
            fn()
        for key in list(self.skip_terms):           # a source nobody asked for its gradient (a leaf of the tape)
            self.settle(key)
        assert not self.skip_terms
        self.s2d_sources.clear()
        self.flush_side()
        if self.finalizers:
            fins, self.finalizers = list(self.finalizers.values()), {}
            if self.side_used:                      # after the weight-gradient kernels, on their stream
                with torch.cuda.stream(_side_stream()):
                    for fn in fins:
                        fn()
            else:
                for fn in fins:
                    fn()
        if self.side_used:
            ev = torch.cuda.Event()
            ev.record(_side_stream())
            torch.cuda.current_stream().wait_event(ev)
            self.side_used = False
        self.side_keep.clear()
        self.ops.clear()
        self.keep.clear()


class SkipTerm(NamedTuple):
    """up(attn) * d skip, not yet added to the gradient of the aggregator's input: gx[b,t,c] += a_up[g,b,t] * gskip[b,c]."""
    a_up: Tensor            # [n_head,B,T,H,W], a workspace buffer of its own (name) until the term is added
    gskip: Tensor           # [B,C,H,W]
    desc: object            # AggDesc
    valid: Optional[Tensor]
    n_head: int
    T: int
    name: str


class Ctx:
    """Per-forward context: parameters by name, parameter-gradient views, scratch, tape, mode flags."""

    def __init__(self, params: Dict[str, Tensor], buffers: Dict[str, Tensor], grads: Optional[Dict[str, Tensor]],
                 ws: Workspace, training: bool, tape: Optional[Tape], eps: float = 1e-5, momentum: float = 0.1,
                 trainable: Optional[Sequence[str]] = None):
        self.p = params
        self.b = buffers
        self.g = grads            # name -> gradient tensor (same shape as the parameter), written by backward
        # names of the parameters that get a gradient; None: all of them, and every op records its full backward as it always
        # has.  Otherwise requires_grad is propagated on the tape (mark / needs): an op output needs a gradient when an input
        # tensor or a parameter of the op does (the model input never does), and the backward skips what nothing needs.
        self.trainable = None if trainable is None else frozenset(trainable)
        self._needs: set = set()  # data pointers of the op outputs that need a gradient (trainable is not None)
        self.ws = ws
        self.training = training
        self.tape = tape
        self.eps = eps
        self.momentum = momentum
        self.device = ws.device
        self._packed: Dict[Tuple, Tensor] = {}
        self._plan_ran = False
        self._gwritten: set = set()
        self.early_hook = None    # TrainStep (data parallel): run by the tape when the backward pass enters the per-frame encoder
        self.want_att = True      # False: the caller never reads the attention masks a forward returns (TrainStep; inference
                                  # without return_att): TimeUNet's full-resolution L-TAE then does not store them
        cus = lib().c2s_device_cus()
        self.cus = cus if cus > 0 else 256

    # -- which tensors need a gradient ---------------------------------------------------------------
    def trains(self, name: Optional[str]) -> bool:
        """Whether parameter `name` gets a gradient."""
        return name is not None and (self.trainable is None or name in self.trainable)

    def needs(self, t: Optional[Tensor]) -> bool:
        """Whether a gradient must flow into tensor `t` (always, when every parameter trains)."""
        return self.trainable is None or (t is not None and t.data_ptr() in self._needs)

    def mark(self, outs: Sequence[Optional[Tensor]], inputs: Sequence[Optional[Tensor]] = (),
             params: Sequence[Optional[str]] = ()) -> bool:
        """requires_grad propagation of one op: True (and the outputs are marked) when the op records a backward, i.e. a tape
        exists and an input tensor needs a gradient or a parameter of the op trains."""
        if self.tape is None:
            return False
        if self.trainable is None:
            return True
        if not (any(self.needs(t) for t in inputs if t is not None) or any(self.trains(n) for n in params)):
            return False
        self._needs.update(o.data_ptr() for o in outs if o is not None)
        return True

    # -- parameter gradient sinks ---------------------------------------------------------------
    def grad_sink(self, name: str) -> Tuple[Tensor, int]:
        """Returns (gradient tensor, accumulate flag) for parameter `name` (a trainable one)."""
        assert self.trains(name), f"grad_sink: {name} is frozen"
        acc = 1 if name in self._gwritten else 0
        self._gwritten.add(name)
        return self.g[name], acc

    def add_param_grad(self, name: str, g: Tensor) -> None:
        dst, acc = self.grad_sink(name)
        if acc:
            check(lib().c2s_add_inplace(dst.data_ptr(), g.data_ptr(), g.numel(), _stream()), "add_inplace")
        else:
            dst.copy_(g.view_as(dst))

    # -- weight packing --------------------------------------------------------------------------
    def _planned(self, key: Tuple, src_ptr: int) -> Optional[Tensor]:
        """Packed weights from the one-launch plan (run at the first pack request of the step), if the plan covers `key`
        for this source pointer; a stale plan (parameters re-allocated) is dropped."""
        plan = self.ws.pack_plan
        if plan is None:
            return None
        hit = plan["outs"].get(key)
        if hit is None or hit[1] != src_ptr:
            self.ws.pack_plan = None
            self.ws.pack_record = {}
            return None
        if not self._plan_ran:
            check(lib().c2s_pack_batch(plan["table"].data_ptr(), plan["njobs"], plan["blocks"], _stream()), "pack_batch")
            self._plan_ran = True
        return hit[0]

    def pack(self, key: Tuple, src: Tensor, src_off: int, cin: int, cout: int, so: int, sc: int, taps: Sequence[int],
             kind: int = 0) -> Tuple[Tensor, int]:
        """Weights packed in the layout `kind` (PACK_KINDS) and the padded output-channel count; cached per forward, taken
        from the step's one-launch plan when it covers `key`, else packed alone and recorded for the next plan.  The filter
        element (o, c, tap t) is src[src_off + o * so + c * sc + taps[t]]."""
        step, floats_fn, pack_fn = PACK_KINDS[kind]
        coutP = (cout + step - 1) // step * step
        hit = self._packed.get(key)
        if hit is not None:
            return hit, coutP
        src_ptr = src.data_ptr() + 4 * src_off
        out = self._planned(key, src_ptr)
        if out is None:
            L_ = lib()
            ntaps = len(taps)
            nfl = ntaps * cin * coutP if kind == 0 else getattr(L_, floats_fn)(cin, coutP)
            out = torch.empty(nfl, device=self.device, dtype=torch.float32)
            lead = (src_ptr, out.data_ptr(), cin, cout, coutP) + ((ntaps,) if kind == 0 else ())
            check(getattr(L_, pack_fn)(*lead, so, sc, _tap_array(taps), _stream()), pack_fn)
            self.ws.pack_record[key] = PackRecord(src_ptr, cin, cout, coutP, ntaps, so, sc, kind, tuple(taps), nfl)
        self._packed[key] = out
        return out, coutP


def _pack_bf16x3(ctx: "Ctx", key: Tuple, src: Tensor, src_off: int, cin: int, cout: int, so: int, sc: int,
                 taps: Sequence[int]) -> Tuple[Tensor, Tensor, int]:
    hit = ctx._packed.get(key)
    coutP = (cout + 31) // 32 * 32
    if hit is not None:
        return hit[0], hit[1], coutP
    n = lib().c2s_bf16x3_packed_elems(cin, coutP)
    whi = torch.empty(n, device=ctx.device, dtype=torch.bfloat16)
    wlo = torch.empty(n, device=ctx.device, dtype=torch.bfloat16)
    check(lib().c2s_pack_weights_bf16x3(src.data_ptr() + 4 * src_off, whi.data_ptr(), wlo.data_ptr(), cin, cout, coutP,
                                        len(taps), so, sc, _tap_array(taps), _stream()), "pack_weights_bf16x3")
    ctx._packed[key] = (whi, wlo)
    return whi, wlo, coutP


# =================================================================================================
# frame flags
# =================================================================================================
def frame_flags(x5: Tensor, pad_value: float) -> Tensor:
    """valid[n] = any(x[n] != pad_value) (reference: utae.py:201-203, temp_shared_block.py:31)."""
    B, T = x5.shape[:2]
    valid = torch.empty(B * T, device=x5.device, dtype=torch.int32)
    check(lib().c2s_frame_flags(x5.data_ptr(), valid.data_ptr(), B * T, x5[0, 0].numel(), float(pad_value), _stream()),
          "frame_flags")
    return valid


# =================================================================================================
# convolutions
# =================================================================================================
# C2S_REDUCE_BATCH=1: the split-K slice sums of all weight gradients of a backward pass in one launch at its end (one slab
# buffer per layer) instead of one launch per layer right behind its weight-gradient kernel.  Measured neutral on the eager
# two-stream step (11.70 vs 11.71 ms), -0.2 ms under hipGraph capture: off by default, switched on by TrainStep.capture().
REDUCE_BATCH = _os.environ.get("C2S_REDUCE_BATCH", "0") != "0"

# The switches of the kernel choice, read by conv_plan whenever a plan is made (tests, tools and bench.py assign them).
# Convolution arithmetic: "f32" = exact fp32 MFMA everywhere (default); "bf16x3" = split-precision bf16 MFMA
# (three products per fp32 product, fp32 accumulate, ~1e-5 relative) for the 3x3 stride-1 forward / data-gradient
# launches whose channel counts are multiples of 8; everything else stays on the exact kernels.
CONV_MODE = _os.environ.get("C2S_CONV_MODE", "f32")
assert CONV_MODE in ("f32", "bf16x3"), CONV_MODE
# fp32 Winograd F(2x2,3x3) for the wide 3x3 layers (forward + data gradient); C2S_WINOGRAD=0 keeps the direct kernel.
WINOGRAD = _os.environ.get("C2S_WINOGRAD", "1") != "0"
# the 8-wave Winograd kernel with the output transform in registers (conv_winograd16.hip) for planes >= 32 wide;
# C2S_WINO16=0 keeps the 4-wave kernel (conv_winograd.hip) everywhere
WINO16 = _os.environ.get("C2S_WINO16", "1") != "0"
# Winograd F(2x2,2x2) over the input parities for the 4x4 stride-2 forward convolutions (conv_s2wino.hip); C2S_S2WINO=0 keeps
# the direct kernel
S2WINO = _os.environ.get("C2S_S2WINO", "1") != "0"


def _use_winograd(K: int, S: int, pad: int, chans: Sequence[int], cout: int, H: int, W: int) -> bool:
    """Winograd F(2x2,3x3) pays off where the 16 transform-domain GEMMs are deep and wide enough."""
    return (WINOGRAD and CONV_MODE == "f32" and K == 3 and S == 1 and pad == 1 and sum(chans) >= 32 and cout >= 64
            and H % 2 == 0 and W % 4 == 0 and W >= 8 and (len(chans) == 1 or chans[0] % 8 == 0))


def _wide_winograd(H: int, W: int, chans: Sequence[int]) -> bool:
    """c2s_conv3x3_winograd16_supported on top of _use_winograd: planes >= 32 wide, at least four chunks of 8 channels,
    whole chunks in every source (ragged channel counts stay on the 4-wave kernel, whose channel index is range-checked)."""
    return WINO16 and W >= 32 and H >= 8 and sum(chans) > 24 and all(c % 8 == 0 for c in chans)


def _use_bf16x3(K: int, S: int, pad: int, chans: Sequence[int]) -> bool:
    return CONV_MODE == "bf16x3" and K == 3 and S == 1 and pad == 1 and all(c % 8 == 0 for c in chans)


def _xpair_taps(py: int) -> List[int]:
    """4x4 weight taps of the transposed stride-2 convolution for output-row parity py, ordered [px][ty][tx]."""
    return [((3 - py) - 2 * ty) * 4 + ((3 - px) - 2 * tx) for px in range(2) for ty in range(2) for tx in range(2)]


# (str_conv_k, str_conv_p) of the stride-2 down / up convolutions besides the default (4, 1): their data gradients and the
# transposed forward run as four stride-1 parity sub-convolutions of (k/2)x(k/2) taps on the implicit-GEMM kernel
PARITY_GEOMETRIES = ((2, 0), (6, 2))


def _parity_taps(K: int, pad: int, py: int, px: int) -> List[int]:
    """Taps of the (K/2)x(K/2) parity sub-kernel (stride 1, pad pad/2, output rows 2*a + py) of a stride-2 transposed
    convolution with kernel K and padding pad = K/2 - 1: sub-tap t reads row a - pad/2 + t through kernel row
    py + 2*pad - 2*t.  Ordered [ty][tx] as the sub-kernel's taps."""
    kp = K // 2
    return [(py + 2 * pad - 2 * ty) * K + (px + 2 * pad - 2 * tx) for ty in range(kp) for tx in range(kp)]


def _conv_desc(*, N: int, C0: int, C1: int = 0, Hin: int, Win: int, Cout: int, CoutP: int, Hout: int, Wout: int, K: int,
               S: int = 1, pad: int, pad_x: Optional[int] = None, pad_mode: int = _lib.PAD_ZEROS, OutH: Optional[int] = None,
               OutW: Optional[int] = None, osy: int = 1, osx: int = 1, ooy: int = 0, oox: int = 0, accumulate: int = 0,
               reflect_adjoint: int = 0) -> ConvDesc:
    """ConvDesc of a square kernel; by default the output is dense (OutH x OutW = Hout x Wout, no placement stride or
    offset), overwritten, padded alike in both directions, without the reflect adjoint."""
    return ConvDesc(N, C0, C1, Hin, Win, Cout, CoutP, Hout, Wout, Hout if OutH is None else OutH,
                    Wout if OutW is None else OutW, K, K, S, pad, pad if pad_x is None else pad_x, pad_mode, osy, osx, ooy, oox,
                    accumulate, reflect_adjoint)


class ConvLaunch(NamedTuple):
    """One launch of a plan: its descriptor, and its weights as Ctx.pack takes them.  `key` follows the weight's name in the
    pack key; filter element (o, c, tap t) is weight[off + o * so + c * sc + taps[t]]."""
    desc: ConvDesc
    key: Tuple
    kind: int               # PACK_KINDS (bf16x3: padded as kind 0, packed by _pack_bf16x3 into a hi / lo pair)
    off: int
    cin: int
    cout: int
    so: int
    sc: int
    taps: Tuple[int, ...]


class ConvPlan(NamedTuple):
    family: str             # key of CONV_FAMILIES
    launches: Tuple[ConvLaunch, ...]


# family -> (entry point, takes a second source, takes a bias, bracketed by PROFILE); after the descriptor every entry point
# takes: source(s), packed weights (bf16x3: hi and lo), bias if any, output, frame flags, stream
CONV_FAMILIES = {
    "wino16": ("c2s_conv3x3_winograd16", True, True, True),             # 8-wave Winograd F(2x2,3x3)
    "wino4": ("c2s_conv3x3_winograd", True, True, True),                # 4-wave Winograd F(2x2,3x3)
    "bf16x3": ("c2s_conv3x3_bf16x3", True, True, False),
    "s2wino": ("c2s_conv4x4s2_winograd", False, True, False),           # F(2x2,2x2), 4x4 stride-2 forward
    "s2dgrad": ("c2s_conv4x4s2_dgrad_winograd", False, False, False),   # F(2x2,2x2), 4x4 stride-2 data gradient
    "smallcin": ("c2s_conv3x3_smallcin", False, True, False),           # the first layer
    "igemm": ("c2s_conv_igemm", True, True, True),
    "xpair": ("c2s_conv_xpair", False, True, False),                    # transposed 4x4 stride-2 rows, one launch per row parity
    "parity": ("c2s_conv_igemm", True, True, True),                     # PARITY_GEOMETRIES: four stride-1 sub-convolutions
}


def _launch(kind: int, key: Tuple, off: int, cin: int, cout: int, so: int, sc: int, taps: Sequence[int], **desc) -> ConvLaunch:
    """One launch that reads `cin` channels (all from one source unless C0 / C1 say otherwise) and writes `cout`, padded as
    the pack kind pads them."""
    step = PACK_KINDS[kind][0]
    return ConvLaunch(_conv_desc(**{"C0": cin, **desc}, Cout=cout, CoutP=(cout + step - 1) // step * step),
                      key, kind, off, cin, cout, so, sc, tuple(taps))


def _transposed_launches(family: str, key: Tuple, off: int, cin: int, cout: int, so: int, sc: int, K: int, pad: int, N: int,
                         H: int, W: int, accumulate: int, radj: int) -> ConvPlan:
    """out (2H x 2W) = stride-2 transposed convolution of an H x W plane with kernel K, padding pad: "xpair" (K = 4) one
    launch per output-row parity, both column parities fused; "parity" four implicit-GEMM launches, where radj folds the
    reflect-pad-2 adjoint into the 3x3 launches (data gradient of a reflect-padded down conv)."""
    plane = dict(N=N, Hin=H, Win=W, Hout=H, Wout=W, OutH=2 * H, OutW=2 * W, osy=2, osx=2, accumulate=accumulate)
    if family == "xpair":
        return ConvPlan(family, tuple(
            _launch(0, key + (py,), off, cin, cout, so, sc, _xpair_taps(py), K=2, pad=1 - py, pad_x=0, ooy=py,
                    reflect_adjoint=radj, **plane) for py in range(2)))
    return ConvPlan(family, tuple(
        _launch(0, key + ("par", py, px), off, cin, cout, so, sc, _parity_taps(K, pad, py, px), K=K // 2, pad=pad // 2, ooy=py,
                oox=px, reflect_adjoint=2 if radj else 0, **plane) for py in range(2) for px in range(2)))


def _family_3x3(N: int, chans: Sequence[int], cout: int, H: int, W: int, K: int, S: int, pad: int):
    """(family, pack kind, key tag) of the 3x3 stride-1 kernels besides the implicit GEMM for `chans` -> cout channels, or
    None."""
    if _use_winograd(K, S, pad, chans, cout, H, W):
        wide = _wide_winograd(H, W, chans) and N <= 65536       # the 8-wave kernel's frame limit
        return ("wino16", 2, "wino") if wide else ("wino4", 1, "wino")
    # (3-pixel planes stay on the implicit GEMM: the bf16x3 kernel's reflect adjoint keeps one border rule per position, and
    # on a 3-pixel axis both reflected rows fold onto position 1)
    return ("bf16x3", 0, "bx") if _use_bf16x3(K, S, pad, chans) and H != 3 and W != 3 else None


# families whose kernels take the frame index from gridDim.z: their launchers refuse N > C2S_CONV_MAX_FRAMES (include/c2s_hip.h)
Z_FRAME_FAMILIES = ("igemm", "xpair", "parity", "bf16x3")


def conv_plan(op: str, N: int, chans: Sequence[int], Cout: int, Hin: int, Win: int, K: int, S: int, pad: int, pad_mode: int,
              si: int = 0, accumulate: int = 0) -> ConvPlan:
    """_conv_plan, refusing at planning time what the planned family's launcher would refuse for its frame count: a plan
    that comes back launches."""
    plan = _conv_plan(op, N, chans, Cout, Hin, Win, K, S, pad, pad_mode, si, accumulate)
    if N > _lib.CONV_MAX_FRAMES and plan.family in Z_FRAME_FAMILIES:
        raise C2SError(f"conv_plan({op!r}): {CONV_FAMILIES[plan.family][0][4:]}: more than {_lib.CONV_MAX_FRAMES} frames in one "
                       f"launch (N = {N}): the frame index is gridDim.z")
    return plan


def _conv_plan(op: str, N: int, chans: Sequence[int], Cout: int, Hin: int, Win: int, K: int, S: int, pad: int, pad_mode: int,
               si: int = 0, accumulate: int = 0) -> ConvPlan:
    """The kernel family of one convolution and its launches: descriptors and pack requests, host integers only (no tensor,
    no Ctx, no stream; the library is asked for its host-side *_supported predicates).  _run_conv executes a plan.
    op "fwd": nn.Conv2d(K, S, pad, pad_mode) of N frames of Hin x Win over the channel concatenation of sources with `chans`
    channels; "dgrad": its data gradient into source `si`, added to what that buffer holds if `accumulate`;
    "tfwd": nn.ConvTranspose2d(K, 2, pad) from chans[0] to Cout channels, Hin x Win -> 2 Hin x 2 Win; "tdgrad": its data
    gradient."""
    KK, Cin = K * K, sum(chans)
    if op == "tfwd":
        return _transposed_launches("xpair" if K == 4 else "parity", ("fwd",), 0, Cin, Cout, KK, Cout * KK, K, pad, N, Hin, Win,
                                    0, 0)
    if op == "tdgrad":
        return ConvPlan("igemm", (_launch(0, ("dgrad",), 0, Cout, Cin, Cout * KK, KK, range(KK), N=N, Hin=2 * Hin, Win=2 * Win,
                                          Hout=Hin, Wout=Win, K=K, S=2, pad=pad, accumulate=accumulate),))
    Ho, Wo = (Hin + 2 * pad - K) // S + 1, (Win + 2 * pad - K) // S + 1
    if op == "fwd":
        def fwd(family, kind, *key):
            return ConvPlan(family, (_launch(kind, ("fwd",) + key, 0, Cin, Cout, Cin * KK, KK, range(KK), N=N,
                                             C0=chans[0], C1=Cin - chans[0], Hin=Hin, Win=Win, Hout=Ho, Wout=Wo, K=K, S=S, pad=pad,
                                             pad_mode=pad_mode),))
        pick = _family_3x3(N, chans, Cout, Hin, Win, K, S, pad)
        if pick:
            return fwd(*pick)
        if S2WINO and CONV_MODE == "f32" and K == 4 and S == 2 and Cin == chans[0]:
            plan = fwd("s2wino", 3, "s2w")
            if lib().c2s_conv4x4s2_winograd_supported(C.byref(plan.launches[0].desc)):
                return plan
        plan = fwd("igemm", 0)
        first = lib().c2s_conv3x3_smallcin_supported(C.byref(plan.launches[0].desc))
        return plan._replace(family="smallcin") if first else plan
    assert op == "dgrad", op
    # the gradient of the output (Cout channels, Ho x Wo) into the Cs channels of source si, which start at channel c_lo
    Cs, c_lo = chans[si], sum(chans[:si])
    radj = 1 if (pad_mode == _lib.PAD_REFLECT and pad > 0) else 0   # reflection adjoint folded into the kernel
    w = (c_lo * KK, Cout, Cs, KK, Cin * KK)

    def dgrad(family, kind, key, taps, **desc):
        return ConvPlan(family, (_launch(kind, ("dgrad",) + key, *w, taps, N=N, Hin=Ho, Win=Wo, Hout=Hin, Wout=Win,
                                         accumulate=accumulate, reflect_adjoint=radj, **desc),))
    if S == 1:
        taps = [(K - 1 - ky) * K + (K - 1 - kx) for ky in range(K) for kx in range(K)]
        pick = _family_3x3(N, [Cout], Cs, Hin, Win, K, S, pad)
        if pick:
            return dgrad(pick[0], pick[1], (pick[2], si), taps, K=K, pad=1)
        return dgrad("igemm", 0, (si,), taps, K=K, pad=K - 1 - pad)
    assert S == 2 and Hin == 2 * Ho and Win == 2 * Wo, (K, S, pad, Hin, Win)
    if (K, pad) in PARITY_GEOMETRIES:
        return _transposed_launches("parity", ("dgrad", si), *w, K, pad, N, Ho, Wo, accumulate, radj)
    assert K == 4 and pad == 1, (K, pad)
    plan = dgrad("s2dgrad", 4, ("s2d", si), range(KK), K=4, S=2, pad=1)     # (cin = gy channels, cout = channels of the source)
    if S2WINO and CONV_MODE == "f32" and lib().c2s_conv4x4s2_dgrad_winograd_supported(C.byref(plan.launches[0].desc)):
        return plan
    return _transposed_launches("xpair", ("dgrad", si), *w, K, pad, N, Ho, Wo, accumulate, radj)


# bench.py sets PROFILE = {"match": {field: value}, "events": []}: launches whose descriptor matches are bracketed
# with HIP events on the launch stream (the stream the kernel runs on) for the live roofline measurement.
PROFILE: Optional[dict] = None


def _run_conv(ctx: Ctx, plan: ConvPlan, wname: str, weight: Tensor, src0: Tensor, src1: Optional[Tensor],
              bias: Optional[Tensor], out: Tensor, valid: Optional[Tensor]) -> None:
    """Execute a plan: per launch, the packed weights of `weight` (ctx.p[wname]), then the family's entry point."""
    entry, two_sources, has_bias, profiled = CONV_FAMILIES[plan.family]
    for desc, key, kind, *where in plan.launches:
        request = ((wname,) + key, weight, *where)
        packed = _pack_bf16x3(ctx, *request)[:2] if plan.family == "bf16x3" else ctx.pack(*request, kind=kind)[:1]
        args = [src0.data_ptr()] + ([_ptr(src1)] if two_sources else []) + [t.data_ptr() for t in packed] + \
            ([_ptr(bias)] if has_bias else []) + [out.data_ptr(), _ptr(valid), _stream()]
        prof = PROFILE
        timed = profiled and prof is not None and all(getattr(desc, k) == v for k, v in prof["match"].items())
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        check(getattr(lib(), entry)(C.byref(desc), *args), entry[4:])
        if timed:
            e1.record()
            prof["events"].append((e0, e1))


def _wgrad_slices(ctx: Ctx, N: int, Hout: int, Wout: int, S: int, cin: int, cout: int) -> int:
    TP = 64 if S == 2 else 128
    l2 = 5
    while l2 > 2 and (1 << l2) > Wout:
        l2 -= 1
    PC = 1 << l2
    ntiles = N * ((Wout + PC - 1) // PC) * ((Hout + TP // PC - 1) // (TP // PC))
    blocks = ((cin + 31) // 32) * ((cout + 63) // 64)
    return max(1, min(ntiles, (2 * ctx.cus) // blocks))     # 2 resident workgroups per CU


def _wgrad(ctx: Ctx, srcs: Sequence[Tensor], gout: Tensor, Cout: int, Hout: int, Wout: int, K: int, S: int, pad: int,
           pad_mode: int, dst: Tensor, so: int, sc: int, taps: Sequence[int], accumulate: int,
           valid: Optional[Tensor]) -> None:
    """Weight gradient of a convolution into `dst` (split-K slabs + fixed-order slice sum), on the side stream."""
    if ctx.tape is not None and _side_ok():
        ctx.tape.defer(lambda: _wgrad_launch(ctx, srcs, gout, Cout, Hout, Wout, K, S, pad, pad_mode, dst, so, sc, taps,
                                             accumulate, valid), [gout, *srcs])
        if srcs[0].shape[0] * Hout * Wout >= SIDE_FLUSH_POSITIONS:
            ctx.tape.flush_side()       # very large layers (TimeUNet's 8M-position planes) come last in the backward pass: start
                                        # them now instead of after the rest of the batch.  (Round 3: with the one-pass norm
                                        # kernels the U-TAE layers of 2M positions run 0.15 ms/step better batched: 1<<22.)
    else:
        _wgrad_launch(ctx, srcs, gout, Cout, Hout, Wout, K, S, pad, pad_mode, dst, so, sc, taps, accumulate, valid)


def _wgrad_desc(ctx: Ctx, srcs: Sequence[Tensor], Cout: int, Hout: int, Wout: int, K: int, S: int, pad: int,
                pad_mode: int) -> WgradDesc:
    """The descriptor of a weight-gradient launch (c2s_wgrad_path answers which kernel it reaches)."""
    N, C0, Hin, Win = srcs[0].shape
    C1 = srcs[1].shape[1] if len(srcs) > 1 else 0
    return WgradDesc(N, C0, C1, Hin, Win, Cout, Hout, Wout, K, K, S, pad, pad, pad_mode,
                     _wgrad_slices(ctx, N, Hout, Wout, S, C0 + C1, Cout))


def _wgrad_launch(ctx: Ctx, srcs: Sequence[Tensor], gout: Tensor, Cout: int, Hout: int, Wout: int, K: int, S: int, pad: int,
                  pad_mode: int, dst: Tensor, so: int, sc: int, taps: Sequence[int], accumulate: int,
                  valid: Optional[Tensor]) -> None:
    s0 = srcs[0]
    s1 = srcs[1] if len(srcs) > 1 else None
    d = _wgrad_desc(ctx, srcs, Cout, Hout, Wout, K, S, pad, pad_mode)
    nfl = lib().c2s_wgrad_workspace_floats(C.byref(d))
    batched = REDUCE_BATCH and ctx.tape is not None
    # batched slice sums: one slab buffer per weight and write (they all live until the end of the backward pass); an
    # accumulating sum is ordered after the batch, which holds the first write of the same weight
    tag = f":acc{len(ctx.ws.reduce_post)}" if accumulate else ""
    slabs = ctx.ws.get(f"wgrad_slabs:{dst.data_ptr()}:{so}:{taps[0]}{tag}" if batched else "wgrad_slabs", nfl)
    check(lib().c2s_conv_wgrad(C.byref(d), s0.data_ptr(), _ptr(s1), gout.data_ptr(), slabs.data_ptr(), slabs.numel(),
                               _ptr(valid), _stream()), "conv_wgrad")
    if batched:
        if accumulate:
            ctx.ws.reduce_post.append((slabs, dst.data_ptr(), so, sc, tuple(taps), d))
        else:
            ctx.ws.reduce_jobs.append((bytes(d), slabs.data_ptr(), dst.data_ptr(), so, sc, tuple(taps), accumulate, d))
        ctx.tape.finalizers[id(ctx.ws)] = ctx.ws.run_reduce_batch
    else:
        check(lib().c2s_wgrad_reduce(C.byref(d), slabs.data_ptr(), dst.data_ptr(), so, sc, _tap_array(taps), accumulate,
                                     _stream()), "wgrad_reduce")


def conv2d(ctx: Ctx, srcs: Sequence[Tensor], wname: str, bname: Optional[str], K: int, S: int, pad: int,
           pad_mode: int, valid: Optional[Tensor], need_input_grad: bool = True) -> Tensor:
    """nn.Conv2d (reference conv.py:70-80, 263-271, 378-382) over the channel concatenation of `srcs`."""
    W = ctx.p[wname]
    Cout, Cin = W.shape[0], W.shape[1]
    s0 = srcs[0]
    s1 = srcs[1] if len(srcs) > 1 else None
    N, C0, Hin, Win = s0.shape
    C1 = s1.shape[1] if s1 is not None else 0
    assert C0 + C1 == Cin, (wname, C0, C1, Cin)
    chans = [C0, C1] if C1 else [C0]
    Ho = (Hin + 2 * pad - K) // S + 1
    Wo = (Win + 2 * pad - K) // S + 1
    KK = K * K
    out = torch.empty(N, Cout, Ho, Wo, device=s0.device, dtype=torch.float32)
    _run_conv(ctx, conv_plan("fwd", N, chans, Cout, Hin, Win, K, S, pad, pad_mode), wname, W, s0, s1,
              ctx.p[bname] if bname else None, out, valid)
    if not ctx.mark([out], srcs, [wname, bname]):
        return out
    tape = ctx.tape
    tape.track(out)
    train_w = ctx.trains(wname)
    need_src = [need_input_grad and ctx.needs(src) for src in srcs]
    if AGG_SKIP_TERM and (K, S, pad) == (4, 2, 1):
        for si, src in enumerate(srcs):             # temporal_aggregate's backward may leave its term to this data gradient
            plan = conv_plan("dgrad", N, chans, Cout, Hin, Win, K, S, pad, pad_mode, si, 0) if need_src[si] else None
            if plan is not None and plan.family == "s2dgrad":
                tape.s2d_sources[src.data_ptr()] = (plan.launches[0].desc, _ptr(valid))

    def bwd():
        g = tape.pop_grad(out)
        if g is None:
            return
        if train_w:
            gw, acc = ctx.grad_sink(wname)
            _log("conv2d", wname, "wgrad")
            _wgrad(ctx, srcs, g, Cout, Ho, Wo, K, S, pad, pad_mode, gw, Cin * KK, KK, list(range(KK)), acc, valid)
        for si, src in enumerate(srcs):
            if not need_src[si]:
                continue
            _log("conv2d", wname, "dgrad")
            if src.data_ptr() in tape.skip_terms:
                plan = conv_plan("dgrad", N, chans, Cout, Hin, Win, K, S, pad, pad_mode, si, 0)
                if plan.family == "s2dgrad" and tape.s2d_sources.get(src.data_ptr(), (None, 0))[1] == _ptr(valid):
                    term = tape.take_skip_term(src)
                    desc, key, kind, *where = plan.launches[0]
                    packed = ctx.pack((wname,) + key, W, *where, kind=kind)[0]
                    check(lib().c2s_conv4x4s2_dgrad_winograd_skip(
                        C.byref(desc), g.data_ptr(), packed.data_ptr(), tape.grads[src.data_ptr()].data_ptr(), _ptr(valid),
                        term.a_up.data_ptr(), term.gskip.data_ptr(), term.n_head, term.T, _stream()),
                        "conv4x4s2_dgrad_winograd_skip")
                    continue
            gin, accf = tape.grad_buffer(src)
            _run_conv(ctx, conv_plan("dgrad", N, chans, Cout, Hin, Win, K, S, pad, pad_mode, si, accf), wname, W, g, None, None,
                      gin, valid)

    tape.record(bwd)
    return out


def conv_transpose2d(ctx: Ctx, x: Tensor, wname: str, bname: str, K: int = 4, pad: int = 1) -> Tensor:
    """nn.ConvTranspose2d(k, s=2, p) (reference conv.py:384-390) for (k, p) = (4, 1) and PARITY_GEOMETRIES, as (k/2)x(k/2)
    parity sub-convolutions."""
    Wt = ctx.p[wname]
    Cin, Cout = Wt.shape[0], Wt.shape[1]
    N, _, H, Wd = x.shape
    assert (K, pad) == (4, 1) or (K, pad) in PARITY_GEOMETRIES, (K, pad)
    KK = K * K
    out = torch.empty(N, Cout, 2 * H, 2 * Wd, device=x.device, dtype=torch.float32)
    _run_conv(ctx, conv_plan("tfwd", N, [Cin], Cout, H, Wd, K, 2, pad, _lib.PAD_ZEROS), wname, Wt, x, None, ctx.p[bname], out,
              None)
    if not ctx.mark([out], [x], [wname, bname]):
        return out
    tape = ctx.tape
    tape.track(out)
    train_w, need_x = ctx.trains(wname), ctx.needs(x)

    def bwd():
        g = tape.pop_grad(out)
        if g is None:
            return
        if train_w:
            gw, acc = ctx.grad_sink(wname)
            _log("conv_transpose2d", wname, "wgrad")
            # dW[ci,co,k] = sum x[ci,p] * g[co, 2p+k-pad]  ==  convKxKs2 weight gradient with (input=g, gout=x)
            _wgrad(ctx, [g], x, Cin, H, Wd, K, 2, pad, _lib.PAD_ZEROS, gw, Cout * KK, KK, list(range(KK)), acc, None)
        if not need_x:
            return
        _log("conv_transpose2d", wname, "dgrad")
        gin, accf = tape.grad_buffer(x)
        _run_conv(ctx, conv_plan("tdgrad", N, [Cin], Cout, H, Wd, K, 2, pad, _lib.PAD_ZEROS, 0, accf), wname, Wt, g, None, None,
                  gin, None)

    tape.record(bwd)
    return out


def depthwise_conv2d(ctx: Ctx, x: Tensor, wname: str, K: int, S: int, pad: int, pad_mode: int,
                     valid: Optional[Tensor], bname: Optional[str] = None) -> Tensor:
    """Depthwise part of DepthwiseSeparableConv2D (reference conv.py:18-20; bias-free) and the depthwise convolution of
    MBConv (mbconv.py:71-79; `bname`: its bias, whose gradient the following norm_act(conv_bias=bname) delivers)."""
    W = ctx.p[wname]
    N, Cc, Hin, Win = x.shape
    Ho = (Hin + 2 * pad - K) // S + 1
    Wo = (Win + 2 * pad - K) // S + 1
    out = torch.empty(N, Cc, Ho, Wo, device=x.device, dtype=torch.float32)
    check(lib().c2s_dwconv_fwd(x.data_ptr(), W.data_ptr(), out.data_ptr(), _ptr(valid), N, Cc, Hin, Win, K, S, pad,
                               pad_mode, _stream()), "dwconv_fwd")
    if bname is not None:
        check(lib().c2s_channel_bias_add(out.data_ptr(), ctx.p[bname].data_ptr(), _ptr(valid), N, Cc, Ho * Wo, _stream()),
              "channel_bias_add")
    if not ctx.mark([out], [x], [wname, bname]):
        return out
    tape = ctx.tape
    tape.track(out)
    train_w, need_x = ctx.trains(wname), ctx.needs(x)

    def bwd():
        g = tape.pop_grad(out)
        if g is None:
            return
        if train_w:
            gw, acc = ctx.grad_sink(wname)
            part = ctx.ws.get("dw_partial", N * Cc * K * K)
            tgt = gw if not acc else torch.empty_like(gw)
            _log("depthwise_conv2d", wname, "wgrad")

            def wgrad():
                check(lib().c2s_dwconv_wgrad(x.data_ptr(), g.data_ptr(), part.data_ptr(), tgt.data_ptr(), _ptr(valid), N, Cc,
                                             Hin, Win, K, S, pad, pad_mode, _stream()), "dwconv_wgrad")
                if acc:
                    check(lib().c2s_add_inplace(gw.data_ptr(), tgt.data_ptr(), tgt.numel(), _stream()), "add_inplace")

            if _side_ok():
                tape.defer(wgrad, [x, g, tgt, part])    # side stream, next to the data-gradient chain (part: a later, larger
                                                        # request replaces the workspace buffer before this launch ends)
            else:
                wgrad()
        if not need_x:
            return
        _log("depthwise_conv2d", wname, "dgrad")
        gin, accf = tape.grad_buffer(x)                 # e.g. the residual branch of the block: accumulate in the kernel
        check(lib().c2s_dwconv_dgrad(g.data_ptr(), W.data_ptr(), gin.data_ptr(), _ptr(valid), N, Cc, Hin, Win, K, S, pad,
                                     pad_mode, accf, _stream()), "dwconv_dgrad")

    tape.record(bwd)
    return out


# =================================================================================================
# normalisation (+ReLU, +residual)
# =================================================================================================
# One-pass normalisation (csrc/norm.hip): statistics / sums and the apply step in ONE read of the activation, the waves of a
# group meeting through memory.  C2S_NORM_ONEPASS=0 keeps the two-pass kernels (A/B runs, and the shapes the one-pass
# form does not take fall back to them anyway).
ONEPASS_NORM = _os.environ.get("C2S_NORM_ONEPASS", "1") != "0"
# Small planes: a wave holds too little data for the meeting to pay (tools/norm_bench.py, isolated: 32x32 planes break even,
# 16x16 planes lose 30-140 %).  Inside a step 32x32 planes still win (one launch instead of two per direction: U-TAE 12.26 ->
# 12.11 ms over three A/B runs), 16x16 planes do not (12.10 vs 12.04): planes below 1024 pixels keep the two-pass kernels.
ONEPASS_MIN_HW = int(_os.environ.get("C2S_NORM_ONEPASS_MIN_HW", "1024"))


def norm_act(ctx: Ctx, x: Tensor, prefix: str, kind: int, groups: int, relu: bool, residual: Optional[Tensor],
             valid: Optional[Tensor], pad_value: float = 0.0, conv_bias: Optional[str] = None, affine: bool = True) -> Tensor:
    """GroupNorm / BatchNorm (+ReLU) (+ residual add) on NCHW x.  `conv_bias` names the bias of the convolution
    that produced x: its gradient (= per-channel sum of dx) falls out of the same reduction.  affine=False: no learnable
    gain / shift (nn.InstanceNorm2d): the kernels run with constant ones / zeros and their gradients are discarded."""
    N, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    batch = kind == _lib.NORM_BATCH
    training = 1 if (ctx.training or not batch) else 0
    d = NormDesc(N, Cc, HW, kind, groups if not batch else 1, training if batch else 1, ctx.eps, ctx.momentum)
    if affine:
        gamma, beta = ctx.p[prefix + ".weight"], ctx.p[prefix + ".bias"]
    else:
        gamma = ctx.ws.get(f"ones{Cc}", Cc)
        beta = ctx.ws.get(f"zeros{Cc}", Cc)
        check(lib().c2s_fill(gamma.data_ptr(), Cc, 1.0, _stream()), "fill")
        check(lib().c2s_fill(beta.data_ptr(), Cc, 0.0, _stream()), "fill")
    rm = ctx.b.get(prefix + ".running_mean") if batch else None
    rv = ctx.b.get(prefix + ".running_var") if batch else None
    ngroups = Cc if batch else N * groups
    gstats = torch.empty(ngroups * 2, device=x.device, dtype=torch.float32)
    row_ab = torch.empty(N * Cc * 3, device=x.device, dtype=torch.float32)   # per row: (scale, beta, mean)
    nws = lib().c2s_norm_workspace_floats(C.byref(d))
    ws = ctx.ws.get("norm", nws)
    y = torch.empty_like(x)
    nbt = ctx.b.get(prefix + ".num_batches_tracked") if (batch and ctx.training) else None   # int64, bumped by the kernel
    sync_bytes = (lib().c2s_norm_onepass_sync_bytes(C.byref(d), 1 if valid is not None else 0)
                  if ONEPASS_NORM and HW >= ONEPASS_MIN_HW else 0)
    if sync_bytes:
        sync = ctx.ws.sync_area(sync_bytes)
        check(lib().c2s_norm_fwd_onepass(C.byref(d), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv),
                                         _ptr(nbt), gstats.data_ptr(), row_ab.data_ptr(), _ptr(residual), y.data_ptr(),
                                         int(relu), _ptr(valid), float(pad_value), sync.data_ptr(), sync.numel(), _stream()),
              "norm_fwd_onepass")
    else:
        check(lib().c2s_norm_fwd(C.byref(d), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(rm), _ptr(rv), _ptr(nbt),
                                 gstats.data_ptr(), row_ab.data_ptr(), _ptr(residual), y.data_ptr(), int(relu),
                                 ws.data_ptr(), ws.numel(), _ptr(valid), float(pad_value), _stream()), "norm_fwd")
    pnames = [prefix + ".weight", prefix + ".bias"] if affine else []
    if not ctx.mark([y], [x, residual], pnames + [conv_bias]):
        return y
    tape = ctx.tape
    tape.track(y)
    need_x = ctx.needs(x)
    need_res = residual is not None and ctx.needs(residual)
    # conv_bias trains => x needs a gradient (x is that convolution's output): without one only gamma / beta can train here
    train_gamma, train_beta = [affine and ctx.trains(n) for n in pnames] or [False, False]

    def bwd():
        g = tape.pop_grad(y)
        if g is None:
            return
        if need_res:
            tape.add_grad(residual, g, own=True)      # the residual branch keeps g itself ...
            gx = torch.empty_like(g) if need_x else None   # ... and the norm gradient goes to a fresh buffer (no copy of g)
        else:
            gx = g if need_x else None  # in place
        if not need_x:
            if train_gamma or train_beta:
                # no input gradient: the sums pass and the parameter launch, no apply pass (the one-pass form does the same
                # arithmetic in the same order, so its shapes take this path too)
                _log("norm", prefix, "params")
                wsn = ctx.ws.get("norm", nws)
                check(lib().c2s_norm_bwd(C.byref(d), x.data_ptr(), g.data_ptr(), gamma.data_ptr(), gstats.data_ptr(),
                                         row_ab.data_ptr(), int(relu), None,
                                         ctx.grad_sink(pnames[0])[0].data_ptr() if train_gamma else None,
                                         ctx.grad_sink(pnames[1])[0].data_ptr() if train_beta else None, None,
                                         wsn.data_ptr(), wsn.numel(), _ptr(valid), _stream()), "norm_bwd")
            return
        _log("norm", prefix, "dgrad")
        if affine and ctx.trainable is not None:
            dgamma = ctx.grad_sink(pnames[0])[0] if train_gamma else None
            dbeta = ctx.grad_sink(pnames[1])[0] if train_beta else None
        elif affine:
            dgamma, _ = ctx.grad_sink(prefix + ".weight")
            dbeta, _ = ctx.grad_sink(prefix + ".bias")
        elif ctx.trainable is None:
            dgamma = torch.empty(Cc, device=x.device, dtype=torch.float32)
            dbeta = torch.empty(Cc, device=x.device, dtype=torch.float32)
        else:
            dgamma = dbeta = None                     # affine=False: nothing to discard when not formed at all
        dbias = ctx.grad_sink(conv_bias)[0] if ctx.trains(conv_bias) else None
        want_params = dgamma is not None or dbeta is not None or dbias is not None
        if want_params:
            _log("norm", prefix, "params")

        def norm_bwd(ws_, dg_, db_, dbi_):
            if sync_bytes:
                sync = ctx.ws.sync_area(sync_bytes)
                check(lib().c2s_norm_bwd_onepass(C.byref(d), x.data_ptr(), g.data_ptr(), gamma.data_ptr(), gstats.data_ptr(),
                                                 row_ab.data_ptr(), int(relu), gx.data_ptr(), _ptr(dg_), _ptr(db_), _ptr(dbi_),
                                                 ws_.data_ptr(), ws_.numel(), _ptr(valid), sync.data_ptr(), sync.numel(),
                                                 _stream()), "norm_bwd_onepass")
            else:
                check(lib().c2s_norm_bwd(C.byref(d), x.data_ptr(), g.data_ptr(), gamma.data_ptr(), gstats.data_ptr(),
                                         row_ab.data_ptr(), int(relu), gx.data_ptr(), _ptr(dg_), _ptr(db_), _ptr(dbi_),
                                         ws_.data_ptr(), ws_.numel(), _ptr(valid), _stream()), "norm_bwd")

        if _side_ok() and want_params:
            # the parameter gradients (one wave per channel: a launch that leaves the GPU idle) go to the side stream; their
            # partial sums live in a buffer of their own until the join
            ws2 = torch.empty(nws, device=x.device, dtype=torch.float32)
            norm_bwd(ws2, None, None, None)
            tape.defer(lambda: check(lib().c2s_norm_bwd_params(C.byref(d), ws2.data_ptr(), _ptr(dgamma), _ptr(dbeta),
                                                               _ptr(dbias), _ptr(valid), _stream()), "norm_bwd_params"),
                       [ws2] if affine else [ws2, dgamma, dbeta])     # affine=False: the discarded sums are temporaries too
        else:
            norm_bwd(ctx.ws.get("norm", nws), dgamma, dbeta, dbias)
        tape.add_grad(x, gx)

    bwd.saved = {"group_stats": gstats, "row_ab": row_ab}     # what the forward left for this step (tests read it here)
    tape.record(bwd)
    return y


def squeeze_excite(ctx: Ctx, x: Tensor, prefix: str, valid: Optional[Tensor], pad_value: float = 0.0) -> Tensor:
    """SqueezeAndExcitation (reference squeeze_and_excitation.py:7-30): x * sigmoid(W2 relu(W1 mean_hw(x))) per frame;
    `prefix` names the module (its Linear layers are prefix.sae.1 and prefix.sae.3, bias-free)."""
    W1, W2 = ctx.p[prefix + ".sae.1.weight"], ctx.p[prefix + ".sae.3.weight"]
    N, Cc = x.shape[:2]
    HW = x[0, 0].numel()
    R = Cc // 16
    assert tuple(W1.shape) == (R, Cc) and tuple(W2.shape) == (Cc, R), (prefix, W1.shape, W2.shape)
    dev = x.device
    pooled = torch.empty(N, Cc, device=dev, dtype=torch.float32)
    hidden = torch.empty(N, R, device=dev, dtype=torch.float32)
    scale = torch.empty(N, Cc, device=dev, dtype=torch.float32)
    y = torch.empty_like(x)
    nws = lib().c2s_se_workspace_floats(N, Cc, HW)
    ws = ctx.ws.get("se", nws)
    check(lib().c2s_se_fwd(x.data_ptr(), W1.data_ptr(), W2.data_ptr(), pooled.data_ptr(), hidden.data_ptr(), scale.data_ptr(),
                           y.data_ptr(), _ptr(valid), N, Cc, HW, float(pad_value), ws.data_ptr(), ws.numel(), _stream()), "se_fwd")
    wn = [prefix + ".sae.1.weight", prefix + ".sae.3.weight"]
    if not ctx.mark([y], [x], wn):
        return y
    tape = ctx.tape
    tape.track(y)
    need_x = ctx.needs(x)

    def bwd():
        g = tape.pop_grad(y)
        if g is None:
            return
        # one fused launch (the input gradient in place of g): a frozen weight's gradient is formed into scratch
        (g1, a1), (g2, a2) = [ctx.grad_sink(n) if ctx.trains(n) else (torch.empty_like(ctx.p[n]), 0) for n in wn]
        if ctx.trains(wn[0]) or ctx.trains(wn[1]):
            _log("squeeze_excite", prefix, "params")
        if need_x:
            _log("squeeze_excite", prefix, "dgrad")
        ws_ = ctx.ws.get("se", nws)
        check(lib().c2s_se_bwd(x.data_ptr(), g.data_ptr(), W1.data_ptr(), W2.data_ptr(), pooled.data_ptr(), hidden.data_ptr(),
                               scale.data_ptr(), g.data_ptr(), g1.data_ptr(), g2.data_ptr(), a1, a2, _ptr(valid), N, Cc, HW,
                               ws_.data_ptr(), ws_.numel(), _stream()), "se_bwd")
        if need_x:
            tape.add_grad(x, g)

    tape.record(bwd)
    return y


# =================================================================================================
# temporal aggregation
# =================================================================================================
def temporal_aggregate(ctx: Ctx, x5: Tensor, attn: Tensor, valid: Optional[Tensor], n_head: int,
                       mode: str = "att_group") -> Tensor:
    """TemporalAggregator (reference temporal_aggregator.py:14-77).  att_group: head g weights channel group g;
    att_mean: the head-averaged attention weights every channel; mean: plain mean over the valid frames.  The two
    off-default modes run the same kernels on a derived weight tensor (c2s_attn_head_mean / c2s_frame_mean_weights)."""
    B, T, Cc, H, W = x5.shape
    src_attn = attn
    if mode == "att_mean":
        attn = torch.empty_like(src_attn)
        check(lib().c2s_attn_head_mean(src_attn.data_ptr(), attn.data_ptr(), n_head, src_attn[0].numel(), _stream()), "attn_head_mean")
    elif mode == "mean":
        attn = torch.empty(n_head, B, T, 1, 1, device=x5.device, dtype=torch.float32)
        check(lib().c2s_frame_mean_weights(_ptr(valid), attn.data_ptr(), n_head, B, T, _stream()), "frame_mean_weights")
    elif mode != "att_group":
        raise ValueError(f"agg_mode {mode!r}")
    h, w = attn.shape[-2:]
    d = AggDesc(B, T, Cc, H, W, n_head, h, w)
    out = torch.empty(B, Cc, H, W, device=x5.device, dtype=torch.float32)
    check(lib().c2s_temporal_aggregate_fwd(C.byref(d), x5.data_ptr(), attn.data_ptr(), _ptr(valid), out.data_ptr(),
                                           _stream()), "temporal_aggregate_fwd")
    if not ctx.mark([out], [x5, src_attn if mode != "mean" else None]):
        return out
    tape = ctx.tape
    tape.track(out)
    need_x = ctx.needs(x5)
    # "mean": the weights derive from the frame flags alone (their gradient is formed and dropped when every parameter trains)
    need_a = ctx.needs(src_attn) if mode != "mean" else ctx.trainable is None

    def bwd():
        g = tape.pop_grad(out)
        if g is None:
            return
        key = x5.data_ptr()
        reg = tape.s2d_sources.get(key)
        skip = (AGG_SKIP_TERM and reg is not None and mode in ("att_group", "att_mean") and need_x and need_a
                and key not in tape.grads and key not in tape.skip_terms and reg[1] == _ptr(valid)
                and (reg[0].N, reg[0].Cout, reg[0].Hout, reg[0].Wout) == (B * T, Cc, H, W)
                and lib().c2s_conv4x4s2_dgrad_winograd_skip_supported(C.byref(reg[0]), n_head, T) == 1)
        gx, accx = tape.grad_buffer(x5) if need_x else (None, 0)
        if need_x:
            _log("temporal_aggregate", mode, "dgrad")
        if not need_a:
            gattn = None
        elif mode == "att_group":
            gattn = tape.grad_of(attn)
            if gattn is None:
                gattn = torch.zeros_like(attn)
                tape.grads[attn.data_ptr()] = gattn
        else:
            gattn = torch.zeros_like(attn)          # gradient of the derived weights
        nws = lib().c2s_temporal_aggregate_bwd_workspace_floats(C.byref(d))
        ws = ctx.ws.get("agg", nws)
        if skip:
            # the levels' terms are pending at once, and a captured step must not allocate: a named buffer per pending term
            used = {t.name for t in tape.skip_terms.values()}
            name = next(n for n in (f"agg_a_up:{H}x{W}:{k}" for k in range(len(used) + 1)) if n not in used)
            a_up = ctx.ws.get(name, nws)
            check(lib().c2s_temporal_aggregate_bwd_skip(C.byref(d), x5.data_ptr(), attn.data_ptr(), _ptr(valid), g.data_ptr(),
                                                        gx.data_ptr(), accx, gattn.data_ptr(), a_up.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), _stream()), "temporal_aggregate_bwd_skip")
            tape.skip_terms[key] = SkipTerm(a_up, g, d, valid, n_head, T, name)
        else:
            check(lib().c2s_temporal_aggregate_bwd(C.byref(d), x5.data_ptr(), attn.data_ptr(), _ptr(valid), g.data_ptr(),
                                                   _ptr(gx), accx, _ptr(gattn),
                                                   ws.data_ptr(), ws.numel(), _stream()), "temporal_aggregate_bwd")
        if mode == "att_mean" and need_a:
            tgt, acca = tape.grad_buffer(src_attn)
            check(lib().c2s_attn_head_mean_bwd(gattn.data_ptr(), tgt.data_ptr(), n_head, src_attn[0].numel(), acca, _stream()),
                  "attn_head_mean_bwd")

    tape.record(bwd)
    return out


# =================================================================================================
# L-TAE
# =================================================================================================
def positional_table(dates: Tensor, d: int, period: float) -> Tensor:
    """[B,T] int days -> [B,T,d] sinusoid table, d = d_model / n_head (reference positional_encoding.py:16-33)."""
    dl = dates.to(torch.int64).contiguous()
    pe = torch.empty(*dl.shape, d, device=dl.device, dtype=torch.float32)
    check(lib().c2s_positional_table_ex(dl.data_ptr(), pe.data_ptr(), dl.numel(), float(period), d, _stream()), "positional_table")
    return pe


# "abs_rel_doy" / "abs_rel_linear": use_abs_rel_enc together with use_doy / add_linear (tae.py:407-423): the first encoder
# (kernel mode 1 / 3 on dates[...,0]) plus the AbsolutePositionalEncoder `positional_encoder_abs` on dates[...,1]
PE_MODES = {"rel": 0, "doy": 1, "abs_rel": 2, "linear": 3, "abs_rel_doy": 4, "abs_rel_linear": 5}


def ltae_attention(ctx: Ctx, x5: Tensor, dates: Tensor, valid: Optional[Tensor], prefix: str, n_head: int, d_k: int,
                   d_model: int, period: float, dropout_p: float, with_embedding: bool, seed: int,
                   keep: Optional[Tensor], seed_dev: Optional[Tensor] = None, pe_mode: str = "rel",
                   need_attn: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """_ltae_attention_quads on any map.  The kernels walk the pixels of a sample four at a time (h * w a multiple of 4);
    every pixel is a series of its own, so a map of another size (3 x 3, 2 x 3, 3 x 5: a side of 24 or 40 input pixels at the
    fourth level) runs as the row of its pixels followed by one to three zero pixels.  Those get zero gradients on the way
    back, hence add nothing to a parameter's gradient, and their outputs and input gradients are dropped."""
    B, T, Cc, h, w = x5.shape
    HW = h * w
    rest = (prefix, n_head, d_k, d_model, period, dropout_p, with_embedding, seed, keep, seed_dev, pe_mode, need_attn)
    if HW % 4 == 0:
        return _ltae_attention_quads(ctx, x5, dates, valid, *rest)
    if keep is not None and ctx.training and dropout_p > 0:
        raise NotImplementedError("crop2seg_amd: an explicit attention keep mask needs an L-TAE map of h * w % 4 == 0 pixels; "
                                  f"got {h} x {w}")
    HWp = (HW + 3) // 4 * 4
    tape = ctx.tape
    xp = torch.zeros(B, T, Cc, 1, HWp, device=x5.device, dtype=torch.float32)
    xp[..., :HW].copy_(x5.reshape(B, T, Cc, 1, HW))
    if tape is not None and ctx.needs(x5):
        tape.track(xp)
        if ctx.trainable is not None:
            ctx._needs.add(xp.data_ptr())

        def bwd_in():
            g = tape.pop_grad(xp)
            if g is not None:
                tape.add_grad(x5, g[..., :HW].reshape(x5.shape).contiguous())

        tape.record(bwd_in)
    nops = len(tape.ops) if tape is not None else 0
    outs_p = _ltae_attention_quads(ctx, xp, dates, valid, *rest)
    outs = tuple(None if o is None else o[..., :HW].reshape(*o.shape[:-2], h, w).contiguous() for o in outs_p)
    if tape is not None and len(tape.ops) > nops:       # the kernels recorded their backward: the outputs carry gradients
        pairs = [(o, op) for o, op in zip(outs, outs_p) if o is not None]
        for o, _ in pairs:
            tape.track(o)
        if ctx.trainable is not None:
            ctx._needs.update(o.data_ptr() for o, _ in pairs)

        def bwd_out():
            for o, op in pairs:
                g = tape.pop_grad(o)
                if g is not None:
                    gp = torch.zeros_like(op)
                    gp[..., :HW].copy_(g.reshape(*op.shape[:-2], 1, HW))
                    tape.add_grad(op, gp)

        tape.record(bwd_out)
    return outs


def _ltae_attention_quads(ctx: Ctx, x5: Tensor, dates: Tensor, valid: Optional[Tensor], prefix: str, n_head: int, d_k: int,
                          d_model: int, period: float, dropout_p: float, with_embedding: bool, seed: int,
                          keep: Optional[Tensor], seed_dev: Optional[Tensor] = None, pe_mode: str = "rel",
                          need_attn: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """L-TAE steps 1-6 (reference tae.py:451-481, 738-847).  Returns (emb [B,d_model,h,w] | None, attn [H,B,T,h,w]).
    pe_mode: "rel" = the default sinusoid of the relative dates; "doy" / "abs_rel" / "linear" = the learnable encoders of
    use_doy / use_abs_rel_enc (dates [B,T,2]) / add_linear (tae.py:404-430): the attention kernels then run with a zero
    table and the general table enters next to them (csrc/ltae_pe.hip).
    need_attn=False: the caller never reads the post-dropout weights (TimeUNet_v1 without return_att): where the kernels allow
    it (c2s_ltae_attn_optional) they are not stored -- the returned attn is then None -- and the backward re-derives the
    keep flags from the forward's counter hash."""
    B, T, Cc, h, w = x5.shape
    HW = h * w
    Q = ctx.p[prefix + ".attention_head.Q"]
    Wk = ctx.p[prefix + ".attention_head.fc1_k.weight"]
    bk = ctx.p[prefix + ".attention_head.fc1_k.bias"]
    Wc3 = ctx.p[prefix + ".inconv.weight"]
    bc = ctx.p[prefix + ".inconv.bias"]
    gamma, beta = ctx.p[prefix + ".in_norm.weight"], ctx.p[prefix + ".in_norm.bias"]
    mode = PE_MODES[pe_mode]
    if mode != 0 and (n_head, d_model) != (16, 256):
        raise NotImplementedError("crop2seg_amd: the learnable positional encoders (csrc/ltae_pe.hip) are built for n_head=16, "
                                  f"d_model=256; got n_head={n_head}, d_model={d_model}")
    dev = x5.device
    pe256 = sin256 = d0 = d1 = None
    if mode == 0:
        pe = positional_table(dates, d_model // n_head, period)
    else:
        pe = ctx.ws.get("ltae_pe_zero", B * T * (d_model // n_head))
        check(lib().c2s_fill(pe.data_ptr(), B * T * (d_model // n_head), 0.0, _stream()), "fill")
        dl = dates.to(torch.int64)
        two = mode in (2, 4, 5)                      # dates [B,T,2]: (relative date, day of year)
        kmode = {4: 1, 5: 3}.get(mode, mode)         # the table kernel's mode for the first encoder
        d0 = (dl[..., 0] if two else dl).contiguous()
        d1 = dl[..., 1].contiguous() if two else None
        enc = prefix + (".positional_encoder_abs.fc" if mode == 2 else ".positional_encoder.fc")
        enc2 = prefix + ".positional_encoder_abs.fc" if mode in (4, 5) else None
        peW, peb = ctx.p[enc + ".weight"], ctx.p[enc + ".bias"]
        pe256 = torch.empty(B, T, d_model, device=dev, dtype=torch.float32)
        sin256 = torch.empty(B, T, d_model, device=dev, dtype=torch.float32) if kmode == 3 else None
        bad = ctx.ws.bufs.get("ltae_pe_bad")
        if bad is None:
            bad = ctx.ws.bufs["ltae_pe_bad"] = torch.zeros(1, device=dev, dtype=torch.int32)
        check(lib().c2s_ltae_pe_table(kmode, d0.data_ptr(), _ptr(d1), float(period), peW.data_ptr(), peb.data_ptr(),
                                      pe256.data_ptr(), _ptr(sin256), bad.data_ptr(), B * T, _stream()), "ltae_pe_table")
        if enc2 is not None:
            check(lib().c2s_ltae_pe_abs_add(d1.data_ptr(), ctx.p[enc2 + ".weight"].data_ptr(), ctx.p[enc2 + ".bias"].data_ptr(),
                                            pe256.data_ptr(), bad.data_ptr(), B * T, _stream()), "ltae_pe_abs_add")
    # parameter-only fold: U [n_head,C], s0 [B,T,n_head]; qwk is kept for the adjoint
    U = torch.empty(n_head, Cc, device=dev, dtype=torch.float32)
    s0 = torch.empty(B, T, n_head, device=dev, dtype=torch.float32)
    qwk = torch.empty(n_head, d_model, device=dev, dtype=torch.float32)
    check(lib().c2s_ltae_fold_fwd_ex(Q.data_ptr(), Wk.data_ptr(), bk.data_ptr(), Wc3.data_ptr(), bc.data_ptr(), pe.data_ptr(),
                                     U.data_ptr(), s0.data_ptr(), qwk.data_ptr(), B * T, Cc, n_head, d_k, d_model, _stream()),
          "ltae_fold_fwd")
    if mode != 0:
        check(lib().c2s_ltae_pe_fwd(qwk.data_ptr(), pe256.data_ptr(), None, s0.data_ptr(), None, B, T, HW, 0, _stream()),
              "ltae_pe_fwd")
    Wc = Wc3.view(d_model, Cc)
    p_eff = dropout_p if ctx.training else 0.0
    d = LtaeDesc(B, T, Cc, HW, n_head, d_model, ctx.eps, p_eff, seed, _ptr(keep) if p_eff > 0 else None, _ptr(seed_dev))
    skip_attn = not need_attn and mode == 0 and with_embedding and (
        bool(lib().c2s_ltae_attn_optional(C.byref(d))) if ctx.tape is not None else lib().c2s_ltae_fwd_path(C.byref(d)) == 2)
    attn = None if skip_attn else torch.empty(n_head, B, T, h, w, device=x5.device, dtype=torch.float32)
    if skip_attn and ctx.tape is not None:      # the keep flags of the attention dropout as bits, for the backward pass
        keep_bits = torch.empty(B * HW * n_head, device=x5.device, dtype=torch.int64)
        d.keep_bits = keep_bits.data_ptr()
        ctx.tape.track(keep_bits)
    # softmax before dropout: saved for the backward (and the score scratch of the three-pass streaming kernels and of the
    # time-chunked ones, path 4); a forward
    # without a tape (inference) does not store it: 16*B*T*h*w floats less to write
    need_pre = ctx.tape is not None or lib().c2s_ltae_fwd_path(C.byref(d)) in (1, 4)
    attn_pre = torch.empty(n_head, B, T, h, w, device=x5.device, dtype=torch.float32) if need_pre else None
    emb = torch.empty(B, d_model, h, w, device=x5.device, dtype=torch.float32) if with_embedding else None
    stats = torch.empty(B * HW * n_head * 2, device=x5.device, dtype=torch.float32)
    Ud, s0d = U, s0
    fws = ctx.ws.get("ltae_fwd", lib().c2s_ltae_fwd_workspace_floats(C.byref(d)))
    prof = PROFILE
    timed = prof is not None and "ltae_events" in prof
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib().c2s_ltae_attn_fwd_ws(C.byref(d), x5.data_ptr(), gamma.data_ptr(), beta.data_ptr(), Ud.data_ptr(),
                                     s0d.data_ptr(), Wc.data_ptr(), bc.data_ptr(), pe.data_ptr(), _ptr(valid),
                                     _ptr(attn), _ptr(attn_pre), _ptr(emb), stats.data_ptr(), fws.data_ptr(),
                                     fws.numel(), _stream()), "ltae_fwd")
    if timed:
        e1.record()
        prof["ltae_events"].append((e0, e1))
    if mode != 0 and emb is not None:
        check(lib().c2s_ltae_pe_fwd(None, pe256.data_ptr(), attn.data_ptr(), None, emb.data_ptr(), B, T, HW, 1, _stream()),
              "ltae_pe_fwd")
    fold_names = [prefix + ".attention_head.Q", prefix + ".attention_head.fc1_k.weight",
                  prefix + ".attention_head.fc1_k.bias", prefix + ".inconv.weight", prefix + ".inconv.bias"]
    norm_names = [prefix + ".in_norm.weight", prefix + ".in_norm.bias"]
    pe_names = [] if mode == 0 else [enc + ".weight", enc + ".bias"] + ([] if enc2 is None else [enc2 + ".weight", enc2 + ".bias"])
    if not ctx.mark([emb, attn], [x5], fold_names + norm_names + pe_names):
        return emb, attn
    tape = ctx.tape
    need_x = ctx.needs(x5)
    train_norm = any(ctx.trains(n) for n in norm_names)
    train_fold = any(ctx.trains(n) for n in fold_names + pe_names)
    if d.keep is not None:              # the backward kernels read the explicit keep mask through the descriptor's raw pointer
        tape.track(keep)
    if attn is not None:
        tape.track(attn)
    if emb is not None:
        tape.track(emb)

    def bwd():
        g_attn = tape.pop_grad(attn) if attn is not None else None
        g_emb = tape.pop_grad(emb) if emb is not None else None
        if g_attn is None and g_emb is None:
            return
        # gx None: the input needs no gradient (c2s_ltae_attn_bwd stores none); in_norm frozen as well: no d x kernel at all
        gx = torch.empty_like(x5) if need_x else None
        dev = x5.device
        gU = torch.empty(n_head, Cc, device=dev)
        gs0 = torch.empty(B, T, n_head, device=dev)
        gWc = torch.empty(d_model, Cc, device=dev)
        gbc = torch.empty(d_model, device=dev)
        # the kernels overwrite these outputs: a sink that already holds a gradient gets a scratch tensor, added afterwards
        pending = []

        def sink(name):
            if not ctx.trains(name):                  # frozen: formed into scratch by a launch that runs anyway
                return torch.empty_like(ctx.p[name])
            dst, acc = ctx.grad_sink(name)
            if not acc:
                return dst
            tmp = torch.empty_like(dst)
            pending.append((dst, tmp))
            return tmp

        ggam = sink(norm_names[0]) if train_norm else None
        gbet = sink(norm_names[1]) if train_norm else None
        if need_x:
            _log("ltae", prefix, "dgrad")
        if train_norm or train_fold:
            _log("ltae", prefix, "params")
        nws = lib().c2s_ltae_bwd_workspace_floats(C.byref(d))
        ws = ctx.ws.get("ltae", nws)
        if mode != 0 and g_emb is not None:          # the positional part of the values: g_a += <g_emb_h, pe_h>
            g_tot = torch.empty_like(attn)
            check(lib().c2s_ltae_pe_gattn(g_emb.data_ptr(), pe256.data_ptr(), _ptr(g_attn), g_tot.data_ptr(), B, T, HW,
                                          _stream()), "ltae_pe_gattn")
            g_attn = g_tot
        check(lib().c2s_ltae_attn_bwd(C.byref(d), x5.data_ptr(), gamma.data_ptr(), beta.data_ptr(), Ud.data_ptr(),
                                      s0d.data_ptr(), Wc.data_ptr(), bc.data_ptr(), pe.data_ptr(), _ptr(valid),
                                      _ptr(attn), attn_pre.data_ptr(), stats.data_ptr(), _ptr(g_emb), _ptr(g_attn),
                                      _ptr(gx), gU.data_ptr(), gs0.data_ptr(), gWc.data_ptr(), gbc.data_ptr(),
                                      _ptr(ggam), _ptr(gbet), ws.data_ptr(), ws.numel(), _stream()), "ltae_bwd")
        if not train_fold:
            for dst, tmp in pending:
                check(lib().c2s_add_inplace(dst.data_ptr(), tmp.data_ptr(), tmp.numel(), _stream()), "add_inplace")
            if need_x:
                tape.add_grad(x5, gx)
            return
        # adjoint of the parameter fold: final gradients of Q, fc1_k, inconv in one launch (frozen ones into scratch)
        sinks = [ctx.grad_sink(nme) if ctx.trains(nme) else (torch.empty_like(ctx.p[nme]), 0) for nme in fold_names]
        acc_mask = sum((1 << i) for i, (_, acc) in enumerate(sinks) if acc)
        fbw = ctx.ws.get("ltae_fold_bwd", lib().c2s_ltae_fold_bwd_workspace_floats_ex(n_head, d_model))
        check(lib().c2s_ltae_fold_bwd_ex(Q.data_ptr(), Wk.data_ptr(), bk.data_ptr(), Wc3.data_ptr(), bc.data_ptr(), pe.data_ptr(),
                                         qwk.data_ptr(), gU.data_ptr(), gs0.data_ptr(),
                                         gWc.data_ptr() if emb is not None else None, gbc.data_ptr() if emb is not None else None,
                                         *[t.data_ptr() for t, _ in sinks], B * T, Cc, n_head, d_k, d_model, acc_mask,
                                         fbw.data_ptr(), fbw.numel(), _stream()), "ltae_fold_bwd")
        if mode != 0:
            g_pe = torch.empty(B, T, d_model, device=dev, dtype=torch.float32)
            gW = sink(enc + ".weight")
            gb = sink(enc + ".bias")
            check(lib().c2s_ltae_pe_bwd_ex(kmode, d0.data_ptr(), _ptr(d1), Q.data_ptr(), Wk.data_ptr(), qwk.data_ptr(),
                                           pe256.data_ptr(), _ptr(sin256), attn.data_ptr(), _ptr(g_emb), gs0.data_ptr(),
                                           g_pe.data_ptr(), sinks[1][0].data_ptr(), sinks[0][0].data_ptr(), gW.data_ptr(),
                                           gb.data_ptr(), B, T, HW, d_k, _stream()), "ltae_pe_bwd")
            if enc2 is not None:
                gW2 = sink(enc2 + ".weight")
                gb2 = sink(enc2 + ".bias")
                check(lib().c2s_ltae_pe_abs_bwd(d1.data_ptr(), g_pe.data_ptr(), gW2.data_ptr(), gb2.data_ptr(), B * T, _stream()),
                      "ltae_pe_abs_bwd")
        for dst, tmp in pending:
            check(lib().c2s_add_inplace(dst.data_ptr(), tmp.data_ptr(), tmp.numel(), _stream()), "add_inplace")
        if need_x:
            tape.add_grad(x5, gx)

    tape.record(bwd)
    return emb, attn


def dropout_nchw(ctx: Ctx, x: Tensor, p: float, seed: int, keep: Optional[Tensor], seed_dev: Optional[Tensor] = None) -> Tensor:
    """nn.Dropout of the L-TAE MLP (reference tae.py:448); identity in eval mode."""
    if not ctx.training or p <= 0.0:
        return x
    B, Cc = x.shape[:2]
    HW = x[0, 0].numel()
    y = torch.empty_like(x)
    check(lib().c2s_dropout_nchw(x.data_ptr(), y.data_ptr(), B, Cc, HW, p, seed, _ptr(seed_dev), _ptr(keep), _stream()), "dropout")
    if ctx.mark([y], [x]):
        tape = ctx.tape
        tape.track(y)

        def bwd():
            g = tape.pop_grad(y)
            if g is None:
                return
            gx = torch.empty_like(g)
            _log("dropout", "", "dgrad")
            check(lib().c2s_dropout_nchw(g.data_ptr(), gx.data_ptr(), B, Cc, HW, p, seed, _ptr(seed_dev), _ptr(keep), _stream()),
                  "dropout_bwd")
            tape.add_grad(x, gx)

        tape.record(bwd)
    return y


def pixel_group_norm(ctx: Ctx, x: Tensor, prefix: str, groups: int) -> Tensor:
    """out_norm of L-TAE: GroupNorm over channel groups of each pixel (reference tae.py:437-440,488)."""
    B, Cc = x.shape[:2]
    HW = x[0, 0].numel()
    gamma, beta = ctx.p[prefix + ".weight"], ctx.p[prefix + ".bias"]
    y = torch.empty_like(x)
    stats = torch.empty(B * groups * HW * 2, device=x.device, dtype=torch.float32)
    check(lib().c2s_pixel_gn_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), stats.data_ptr(), B, Cc,
                                 HW, groups, ctx.eps, _stream()), "pixel_gn_fwd")
    pn = [prefix + ".weight", prefix + ".bias"]
    if ctx.mark([y], [x], pn):
        tape = ctx.tape
        tape.track(y)
        need_x = ctx.needs(x)

        def bwd():
            g = tape.pop_grad(y)
            if g is None:
                return
            # one fused launch: what nothing needs (a frozen gamma / beta, the input gradient) is formed into scratch
            gx = torch.empty_like(x)
            dg, db = [ctx.grad_sink(n)[0] if ctx.trains(n) else torch.empty_like(ctx.p[n]) for n in pn]
            if ctx.trains(pn[0]) or ctx.trains(pn[1]):
                _log("pixel_group_norm", prefix, "params")
            if need_x:
                _log("pixel_group_norm", prefix, "dgrad")
            nws = lib().c2s_pixel_gn_bwd_workspace_floats(B, Cc, HW)
            ws = ctx.ws.get("pixel_gn", nws)
            check(lib().c2s_pixel_gn_bwd(x.data_ptr(), g.data_ptr(), gamma.data_ptr(), stats.data_ptr(), gx.data_ptr(),
                                         dg.data_ptr(), db.data_ptr(), B, Cc, HW, groups, ws.data_ptr(), ws.numel(),
                                         _stream()), "pixel_gn_bwd")
            if need_x:
                tape.add_grad(x, gx)

        tape.record(bwd)
    return y


# =================================================================================================
# loss / optimiser
# =================================================================================================
def cross_entropy(logits: Tensor, target: Tensor, class_w: Tensor, ws: Workspace, want_grad: bool,
                  label_smoothing: float = 0.0, ignore_index: int = -100) -> Tuple[Tensor, Optional[Tensor]]:
    """nn.CrossEntropyLoss(weight=class_w, label_smoothing=...) (reference train.py:463-468; ignore_index is torch's
    default -100: the reference ignores its last class through a zero class weight).  Returns (loss[1], dlogits | None)."""
    B, K = logits.shape[:2]
    HW = logits[0, 0].numel()
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    gl = torch.empty_like(logits) if want_grad else None
    n = lib().c2s_cross_entropy_workspace_floats(B, HW)
    w = ws.get("ce", n)
    check(lib().c2s_cross_entropy(logits.data_ptr(), target.data_ptr(), class_w.data_ptr(), loss.data_ptr(), _ptr(gl), B,
                                  K, HW, float(label_smoothing), int(ignore_index), w.data_ptr(), w.numel(), _stream()),
          "cross_entropy")
    return loss, gl


def bad_target_count(ws: Workspace) -> int:
    """Targets outside [0, K) (other than ignore_index) the last cross_entropy call on this workspace met: torch's
    CrossEntropyLoss raises on them, the kernel skips and counts them.  Reads a device value (host synchronisation)."""
    w = ws.bufs.get("ce")
    return 0 if w is None else int(float(w[w.numel() - 1]))


def adam_flat(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: int, lr: float = 1e-3, b1: float = 0.9,
              b2: float = 0.999, eps: float = 1e-8, grad_scale: float = 1.0, step_dev: Optional[Tensor] = None) -> None:
    check(lib().c2s_adam_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, b1, b2, eps, step,
                              _ptr(step_dev), grad_scale, _stream()), "adam")


# Guarded optimiser step (csrc/guard.hip; the layout of the status block: include/c2s_hip.h).  All stream-ordered; `status` is
# the float64[4] tensor of guard_status(), `slots` int64 [n, 2] (offset, length), `mask` / `slot_steps` int32 [n].
GUARD_STATUS_BYTES = 32


def guard_status(device) -> Tensor:
    """A zeroed status block; `guard_views` names its fields."""
    return torch.zeros(GUARD_STATUS_BYTES // 8, device=device, dtype=torch.float64)


def guard_views(status: Tensor) -> Dict[str, Tensor]:
    """0-dim views of the status block's fields (no copy, no synchronisation until a value is read)."""
    f, i = status.view(torch.float32), status.view(torch.int32)
    return {"sumsq": status[0], "ok": i[2], "scale": f[3], "norm": f[4], "coef": f[5]}


def grad_sumsq(g: Tensor, slots: Tensor, mask: Tensor, ws: Workspace, status: Tensor) -> None:
    """status.sumsq = sum of squares of the trainable slots of `g`, in float64 and in a fixed order."""
    n = lib().c2s_grad_sumsq_workspace_doubles()
    w = ws.get("grad_sumsq", 2 * n)                      # n doubles (the allocator's blocks are 8-byte aligned)
    check(lib().c2s_grad_sumsq(g.data_ptr(), slots.data_ptr(), mask.data_ptr(), mask.numel(), g.numel(), w.data_ptr(), n,
                               status.data_ptr(), _stream()), "grad_sumsq")


def step_decide(status: Tensor, max_grad_norm: Optional[float], grad_scale: float, skip_nonfinite: bool, mask: Tensor,
                slot_steps: Tensor, skip_count: Tensor) -> None:
    """Clip coefficient and skip decision from status.sumsq; advances `slot_steps` of the trainable slots or `skip_count`."""
    check(lib().c2s_step_decide(status.data_ptr(), 0.0 if max_grad_norm is None else float(max_grad_norm), float(grad_scale),
                                int(bool(skip_nonfinite)), mask.data_ptr(), slot_steps.data_ptr(), mask.numel(),
                                skip_count.data_ptr(), _stream()), "step_decide")


def adam_slots(p: Tensor, g: Tensor, m: Tensor, v: Tensor, slots: Tensor, mask: Tensor, slot_steps: Tensor, status: Tensor,
               lr: float = 1e-3, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8) -> None:
    """`adam_flat` over every trainable slot in one launch: per-slot step counts, gradient scale and go-ahead from `status`."""
    check(lib().c2s_adam_slots(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), slots.data_ptr(), mask.data_ptr(),
                               slot_steps.data_ptr(), mask.numel(), p.numel(), lr, b1, b2, eps, status.data_ptr(), _stream()),
          "adam_slots")


def restore_if_skipped(dst: Tensor, saved: Tensor, status: Tensor) -> None:
    """dst = saved where the step was skipped (status.ok == 0); untouched otherwise."""
    check(lib().c2s_restore_if_skipped(dst.data_ptr(), saved.data_ptr(), dst.numel(), status.data_ptr(), _stream()),
          "restore_if_skipped")


# Learning-rate schedule and per-slot hyper-parameters on the device (csrc/guard.hip; the layout of the schedule block:
# include/c2s_hip.h).  `sched` is the int32[4] tensor of sched_state(), `table` float32 [n], `hp` float32 [nslots, 2] =
# (lr multiplier, weight decay); `status` None = an unguarded step.
SCHED_STATE_BYTES = 16


def sched_state(device, t: int = 0, scale: float = 1.0) -> Tensor:
    """A schedule block at position `t` with `scale`; `sched_views` names its fields (host -> device copy: not under capture)."""
    host = torch.zeros(SCHED_STATE_BYTES // 4, dtype=torch.int32)
    host[0] = int(t)
    host.view(torch.float32)[1] = float(scale)
    return host.to(device)


def sched_views(sched: Tensor) -> Dict[str, Tensor]:
    """0-dim views of the schedule block's fields (no copy, no synchronisation until a value is read)."""
    f = sched.view(torch.float32)
    return {"t": sched[0], "scale": f[1], "lr_now": f[2]}


def lr_advance(sched: Tensor, table: Tensor, mask: Tensor, slot_steps: Tensor, status: Optional[Tensor] = None) -> None:
    """On an applied step: sched.lr_now = table[min(t, n - 1)] * scale, t += 1; without `status` also the trainable slots'
    step counts (a guarded step's step_decide has advanced them)."""
    check(lib().c2s_lr_advance(sched.data_ptr(), table.data_ptr(), table.numel(), mask.data_ptr(), slot_steps.data_ptr(),
                               mask.numel(), _ptr(status), _stream()), "lr_advance")


def adam_slots_hp(p: Tensor, g: Tensor, m: Tensor, v: Tensor, slots: Tensor, mask: Tensor, slot_steps: Tensor, hp: Tensor,
                  sched: Tensor, status: Optional[Tensor] = None, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8,
                  decoupled: bool = False, grad_scale: float = 1.0) -> None:
    """`adam_slots` with the rate sched.lr_now * hp[s, 0] and the weight decay hp[s, 1] per slot, coupled (torch.optim.Adam) or
    decoupled (torch.optim.AdamW).  Without `status` the step is always applied, the gradient scaled by `grad_scale`."""
    check(lib().c2s_adam_slots_hp(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), slots.data_ptr(), mask.data_ptr(),
                                  slot_steps.data_ptr(), hp.data_ptr(), mask.numel(), p.numel(), sched.data_ptr(), b1, b2, eps,
                                  int(bool(decoupled)), float(grad_scale), _ptr(status), _stream()), "adam_slots_hp")


# Training-state snapshots (csrc/snapshot.hip; blob and status layouts: include/c2s_hip.h).  All stream-ordered.  The layout is
# planned by checkpoint.plan_layout (pure host code); `snapshot_table` turns it into the device table.
SNAPSHOT_HEADER_BYTES = 64
SNAPSHOT_STATUS_BYTES = 32
SNAPSHOT_SPAN_BYTES = 8192
SNAPSHOT_MAX_BLOCKS = 1024
SNAPSHOT_MAGIC = 0x53533243
SNAPSHOT_VERSION = 1


def snapshot_table(ptrs: Sequence[int], nbytes: Sequence[int], offsets: Sequence[int], device) -> Tensor:
    """The region table of c2s_snapshot_gather / c2s_snapshot_scatter: filled on the host, uploaded once (host -> device
    copy: call outside hipGraph capture)."""
    L_ = lib()
    rec = L_.c2s_snapshot_job_bytes()
    table = torch.zeros(max(len(ptrs), 1) * rec, dtype=torch.uint8)
    block = 0
    for i, (p, n, o) in enumerate(zip(ptrs, nbytes, offsets)):
        check(L_.c2s_snapshot_job_fill(table.data_ptr() + i * rec, p if n else None, n, o, block), "snapshot_job_fill")
        block += L_.c2s_snapshot_job_blocks(n)
    return table.to(device)


def snapshot_status(device) -> Tensor:
    """A zeroed status block as int64[4]: ok = int32 word 0, reason = int32 word 1, the recomputed sums = words 1 and 2."""
    return torch.zeros(SNAPSHOT_STATUS_BYTES // 8, device=device, dtype=torch.int64)


def snapshot_gather(table: Tensor, nregions: int, blob: Tensor) -> None:
    """Every live region into `blob` (uint8, header + payload), the header's sums from the same reads."""
    check(lib().c2s_snapshot_gather(table.data_ptr(), nregions, blob.data_ptr(), blob.numel() * blob.element_size(), _stream()),
          "snapshot_gather")


def snapshot_verify(blob: Tensor, nregions: int, status: Tensor) -> None:
    """status.ok = 1 iff the blob's header fits `nregions` and the blob's size and both sums agree with the payload."""
    check(lib().c2s_snapshot_verify(blob.data_ptr(), blob.numel() * blob.element_size(), nregions, status.data_ptr(), _stream()),
          "snapshot_verify")


def snapshot_scatter(table: Tensor, nregions: int, blob: Tensor, status: Tensor) -> None:
    """`blob` back into the live regions where status.ok == 1; nothing is written otherwise."""
    check(lib().c2s_snapshot_scatter(table.data_ptr(), nregions, blob.data_ptr(), blob.numel() * blob.element_size(),
                                     status.data_ptr(), _stream()), "snapshot_scatter")
