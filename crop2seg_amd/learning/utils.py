"""Harness pieces that sit directly on the hot path (reference src/learning/utils.py:50-136, 312-328;
src/learning/weight_init.py:4-46; train.py:454,463-468): model selection, weight initialisation and the
train step  zero_grad -> forward -> CrossEntropy -> backward -> (gradient all-reduce) -> Adam.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.init as init

from .. import engine as E
from ..backbones import functional as Fn
from ..backbones.modules import UTAE, WTAE, TimeUNet_v1

Tensor = torch.Tensor

# Two-bucket gradient exchange overlapped with the encoder's backward pass (TrainStep._forward_backward); C2S_DDP_OVERLAP=0
# keeps the single all-reduce after the backward pass.
OVERLAP_EXCHANGE = __import__("os").environ.get("C2S_DDP_OVERLAP", "1") != "0"


def get_model(config):
    """reference src/learning/utils.py:50-136: dispatch on config.model with the same kwarg mapping
    (encoder=False, return_maps=False fixed)."""
    common = dict(
        input_dim=config.input_dim, encoder_widths=config.encoder_widths, decoder_widths=config.decoder_widths,
        out_conv=config.out_conv, str_conv_k=config.str_conv_k, str_conv_s=config.str_conv_s,
        str_conv_p=config.str_conv_p, agg_mode=config.agg_mode, encoder_norm=config.encoder_norm, n_head=config.n_head,
        d_model=config.d_model, d_k=config.d_k, encoder=False, return_maps=False, pad_value=config.pad_value,
        padding_mode=config.padding_mode, conv_type=config.conv_type, use_mbconv=config.use_mbconv,
        add_squeeze_excit=config.add_squeeze, use_abs_rel_enc=config.use_abs_rel_enc, num_queries=config.num_queries,
        use_doy=config.use_doy, add_linear=config.add_linear)
    if config.model == "utae":
        return UTAE(add_boundary_loss=config.add_boundary_loss, **common)
    if config.model == "wtae":
        return WTAE(add_boundary_loss=config.add_boundary_loss, **common)
    if config.model == "timeunet":
        return TimeUNet_v1(**common)
    raise NotImplementedError(f"model {config.model!r}: crop2seg_amd builds utae / wtae / timeunet")


def default_config(model: str = "utae", **overrides):
    """argparse defaults of the reference's train.py:25-186 that reach get_model()."""
    from types import SimpleNamespace
    cfg = dict(model=model, encoder_widths=[64, 64, 64, 128], decoder_widths=[32, 32, 64, 128], out_conv=[32, 15],
               str_conv_k=4, str_conv_s=2, str_conv_p=1, agg_mode="att_group", encoder_norm="group", n_head=16,
               d_model=256, d_k=4, input_dim=10, num_queries=1, pad_value=0, padding_mode="reflect", conv_type="2d",
               use_mbconv=False, add_squeeze=False, use_doy=False, use_abs_rel_enc=False, add_linear=False,
               add_boundary_loss=False, num_classes=15, ignore_index=-1, lr=1e-3, label_smoothing=0.0)
    cfg.update(overrides)
    return SimpleNamespace(**cfg)


def weight_init(m):
    """reference src/learning/weight_init.py:4-46 (the module types that occur in the three backbones)."""
    if isinstance(m, nn.Conv1d):
        init.normal_(m.weight.data)
        if m.bias is not None:
            init.normal_(m.bias.data)
    elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        init.xavier_normal_(m.weight.data)
        if m.bias is not None:
            init.normal_(m.bias.data)
    elif isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
        init.normal_(m.weight.data, mean=0, std=1)
        init.constant_(m.bias.data, 0)
    elif isinstance(m, nn.Linear):
        init.xavier_normal_(m.weight.data)
        if m.bias is not None:
            init.normal_(m.bias.data)


def trainable_runs(offsets: List[int], total: int, flags: List[bool], steps: Optional[List[int]] = None) -> List[Tuple[int, int]]:
    """[start, end) ranges of the flat buffers that cover the trainable parameters: slot i is [offsets[i], offsets[i + 1])
    (the last one ends at `total`), consecutive trainable slots form one run.  With `steps` (the Adam step count of every
    parameter) a run also ends where the step count changes, so that one Adam launch serves it."""
    runs: List[List[int]] = []
    for i, f in enumerate(flags):
        if not f:
            continue
        beg, end = offsets[i], offsets[i + 1] if i + 1 < len(offsets) else total
        key = None if steps is None else steps[i]
        if runs and runs[-1][1] == beg and runs[-1][2] == key and flags[i - 1]:
            runs[-1][1] = end
        else:
            runs.append([beg, end, key])
    return [(b, e) for b, e, _ in runs]


def clip_runs(runs: List[Tuple[int, int]], lo: int, hi: int) -> List[Tuple[int, int]]:
    """The parts of `runs` inside [lo, hi)."""
    return [(max(b, lo), min(e, hi)) for b, e in runs if min(e, hi) > max(b, lo)]


def early_cut(names: List[str], written, flags: List[bool]) -> int:
    """First index of the early bucket of the two-bucket gradient exchange: the longest suffix of `names` whose gradients are
    final when the backward pass enters the per-frame encoder, i.e. every slot in it is in `written` or frozen (flags False:
    never written).  An unwritten trainable slot ends the walk, whatever lies in front of it.  0 (the encoder has nothing left
    to write) and len(names) (nothing final yet) both mean: no early bucket."""
    i = len(names)
    while i > 0 and (names[i - 1] in written or not flags[i - 1]):
        i -= 1
    return i


def slot_table(offsets: List[int], total: int, flags: List[bool]) -> Tuple[List[Tuple[int, int]], List[int]]:
    """The table the guarded step's kernels walk (csrc/guard.hip): (offset, padded length) of every slot of the flat buffers --
    slot i is [offsets[i], offsets[i + 1]), the last one ends at `total` -- and the mask of trainable slots (1 / 0)."""
    if len(offsets) != len(flags):
        raise ValueError("slot_table: one flag per slot")
    ends = list(offsets[1:]) + [total]
    if any(e < b for b, e in zip(offsets, ends)) or (offsets and offsets[0] < 0):
        raise ValueError("slot_table: offsets must ascend and end within `total`")
    return [(b, e - b) for b, e in zip(offsets, ends)], [1 if f else 0 for f in flags]


class TrainStep:
    """One optimiser step of the reference's training loop (src/learning/utils.py:314-328) with everything on
    the HIP engine and no autograd graph:

        zero_grad -> model(x, batch_positions=dates) -> CrossEntropyLoss(weight) -> backward -> Adam.step()

    Parameters, gradients and Adam moments live in three flat fp32 buffers (the module's parameters are
    re-pointed at views of the flat parameter buffer), so data-parallel training needs exactly one all-reduce of
    `flat_grad` per step (RCCL over xGMI; torch.distributed backend "nccl") and the optimiser is one kernel.

    Fine-tuning: a parameter with requires_grad False (read at every eager step; fixed by capture()) gets no gradient, no
    launch of its own and no update.  The flat layout keeps every parameter; Adam and the gradient exchange cover the runs
    of trainable slots, and, as in torch.optim.Adam, a parameter's step count advances only on the steps where it trained.

    Guarded step (`max_grad_norm` and / or `skip_nonfinite`; with both at their defaults the step launches exactly what it
    launched without them).  The L2 norm of the gradient -- over the trainable slots, after the data-parallel sum and its
    1/world scale, so every rank decides alike -- is taken on the device, and one decision launch follows:
      max_grad_norm: torch.nn.utils.clip_grad_norm_(norm_type=2): coef = min(1, max_grad_norm / (norm + 1e-6)) is folded
        into the scale Adam applies; `flat_grad` keeps the unclipped sum.
      skip_nonfinite: if the norm is not finite the step changes nothing, as when torch.optim.Adam.step() is not called:
        parameters, both moments and the per-parameter step counts stay, and the model's floating-point buffers (BatchNorm
        running_mean / running_var, re-pointed at views of one flat tensor) are put back to their values from before this
        step's forward pass.  The integer buffers are not rolled back: `num_batches_tracked` may advance on a skipped step.
      Without skip_nonfinite a non-finite step is applied as before; skip_nonfinite alone uses coef = 1.
    Adam then runs as one launch over all slots with per-slot step counts kept on the device (a skip that falls while a
    parameter is frozen does not count against it).  Nothing inside a step, eager or replayed, synchronises with the host; the
    readers do: `last_grad_norm` / `last_clip_coef` (device scalars of the last decided step), `skipped_steps()`,
    `sync_steps()`.  Until `sync_steps()` the host's `param_steps` / `step_count` count a skipped step as taken.

    `criterion` (the reference's iterate(..., criterion=criterion), train.py:466-474,488).  None: the weighted, label-smoothed
    cross entropy above, launch for launch what the step ran before the argument existed.  Otherwise any object with
    criterion(logits, y, want_grad=True) -> scalar float32 device tensor and grad() -> dL/dlogits: FocalCELoss,
    SmoothCrossEntropy2D (not with reduction='none') and RecallCrossEntropy of learning/losses.py as they are.  The criterion
    then decides about ignored labels and class weights; num_classes / ignore_index / label_smoothing of this constructor
    belong to the default loss only.  It runs eagerly and inside capture() / replay() (it must not synchronise with the
    host).  Data parallel: every rank evaluates the criterion on its own batch -- RecallCrossEntropy weighs by the recall of
    the rank's batch, which is what the reference does under torch DDP; the gradients are averaged as always.

    Schedule, groups and weight decay (with `lr_schedule`, `schedule_steps`, `weight_decay`,
    `decoupled_weight_decay` and `param_groups` at their defaults the step launches exactly what it launched without them).
      lr_schedule: None = the one-entry table [lr]; a sequence of floats = the table, table[t] the rate of the (t+1)-th applied
        step, the last entry held past the end; a callable f(t), evaluated on the host for t in range(schedule_steps)
        (learning/schedules.py: warmup_cosine, from_torch).  The table and the position live on the device, so the rate moves
        under replay(); a skipped step does not advance it.
      weight_decay: torch.optim.Adam(weight_decay=) -- the decay joins the clipped gradient -- or, with
        decoupled_weight_decay=True, torch.optim.AdamW.  A frozen parameter is not decayed.
      param_groups: [{"params": a name prefix | a list of names or prefixes | a predicate on the name, "lr_mult": 1.0,
        "weight_decay": the global one}]; unmatched parameters take lr_mult 1 and the global decay.
    The step then runs c2s_lr_advance and c2s_adam_slots_hp over the guarded step's slot table, guarded or not.  Readers:
    `last_lr` (device scalar), `schedule_position()` (host synchronisation); `set_lr_scale(s)` multiplies every entry from the next
    step on (reduce-on-plateau).  Snapshots carry the position and the scale; the table and the groups are the constructor's.
    """

    def __init__(self, model, num_classes: int = 15, ignore_index: int = -1, lr: float = 1e-3,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, process_group=None,
                 distributed: bool = False, label_smoothing: float = 0.0, boundary_gamma: float = 2.0,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, criterion=None,
                 lr_schedule=None, schedule_steps: Optional[int] = None, weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, param_groups=None):
        self.model = model
        if criterion is not None:
            if not callable(criterion) or not callable(getattr(criterion, "grad", None)):
                raise TypeError("TrainStep: criterion must be callable as criterion(logits, y, want_grad=True) and have grad()")
            if getattr(criterion, "reduction", "mean") == "none":
                raise ValueError("TrainStep: a criterion with reduction='none' has no scalar loss to train on")
        self.criterion = criterion
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"TrainStep: max_grad_norm must be positive or None, got {max_grad_norm!r}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.label_smoothing = float(label_smoothing)       # train.py:172,466-468
        self.boundary_gamma = float(boundary_gamma)         # FocalCELoss(gamma=2.0), src/learning/utils.py:259
        self.num_classes = num_classes
        if model.spec.encoder:
            raise ValueError("TrainStep needs a model with a classification head (encoder=False)")
        self.lr, self.betas, self.eps = lr, betas, eps
        named = list(model.named_parameters())
        self._named = named                             # requires_grad is read off these at every step
        self.names = [n for n, _ in named]
        dev = named[0][1].device
        sizes = [p.numel() for _, p in named]
        # 16-byte aligned slots
        offs, o = [], 0
        for s in sizes:
            offs.append(o)
            o += (s + 3) // 4 * 4
        self.total = o
        self.offsets = offs
        self.param_steps = [0] * len(named)             # Adam step count per parameter (advances only where it trained)
        self.flat_param = torch.zeros(o, device=dev, dtype=torch.float32)
        self.flat_grad = torch.zeros(o, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(o, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(o, device=dev, dtype=torch.float32)
        self.params: Dict[str, Tensor] = {}
        self.grads: Dict[str, Tensor] = {}
        for (n, p), off, s in zip(named, offs, sizes):
            view = self.flat_param[off:off + s].view_as(p)
            view.copy_(p.data)
            p.data = view                               # module parameters now alias the flat buffer
            self.params[n] = view
            self.grads[n] = self.flat_grad[off:off + s].view_as(p)
        cw = torch.ones(num_classes, device=dev, dtype=torch.float32)
        cw[ignore_index] = 0                            # train.py:463-464
        self.class_w = cw
        self.step_count = 0
        self.ws = E.Workspace(dev)
        # schedule / groups / weight decay: on when any of the five arguments is non-default
        self.hp = (lr_schedule is not None or schedule_steps is not None or float(weight_decay) != 0.0
                   or bool(decoupled_weight_decay) or param_groups is not None)
        if self.guarded:
            self._init_guard(dev)
        if self.hp:
            self._init_hp(dev, lr_schedule, schedule_steps, weight_decay, decoupled_weight_decay, param_groups)
        self.dp = None
        if distributed:
            from .ddp import FlatDataParallel
            self.dp = FlatDataParallel(process_group)
            # identical initial weights AND BatchNorm buffers on every rank
            self.dp.sync_parameters(self.flat_param, [b for _, b in model.named_buffers()])

    # ------------------------------------------------------------------------------------------------ guarded step
    def _init_guard(self, dev) -> None:
        """Device state of the guarded step: slot table, mask, per-slot step counts, status block, skip counter; with
        skip_nonfinite also the model's floating-point buffers as views of one flat tensor, and its copy."""
        self._init_slots(dev)
        self._status = E.guard_status(dev)
        self._skip_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        views = E.guard_views(self._status)
        self.last_grad_norm, self.last_clip_coef = views["norm"], views["coef"]
        self._attempts = 0
        self.flat_buf = self._buf_saved = None
        if self.skip_nonfinite:
            fbufs = [b for _, b in self.model.named_buffers() if b.is_floating_point()]
            n = sum((b.numel() + 3) // 4 * 4 for b in fbufs)
            self.flat_buf = torch.zeros(n, device=dev, dtype=torch.float32)
            self._buf_saved = torch.zeros(n, device=dev, dtype=torch.float32)
            o = 0
            for b in fbufs:
                if b.dtype != torch.float32:
                    raise ValueError("TrainStep(skip_nonfinite=True): floating-point buffers must be float32")
                view = self.flat_buf[o:o + b.numel()].view_as(b)
                view.copy_(b.data)
                b.data = view                           # the module's buffers now alias the flat tensor
                o += (b.numel() + 3) // 4 * 4

    def _init_slots(self, dev) -> None:
        """Slot table, mask and per-slot step counts on the device: shared by the guarded step and the schedule path."""
        if getattr(self, "_slots_dev", None) is not None:
            return
        table, _ = slot_table(self.offsets, self.total, [True] * len(self.offsets))
        self._slots_dev = torch.tensor(table, device=dev, dtype=torch.int64)
        self._mask_dev = torch.zeros(len(table), device=dev, dtype=torch.int32)
        self._mask_flags: Optional[List[bool]] = None            # the flags `_mask_dev` holds
        self.slot_steps_dev = torch.tensor(self.param_steps, device=dev, dtype=torch.int32)

    # ------------------------------------------------------------------- schedule, groups and weight decay
    def _init_hp(self, dev, lr_schedule, schedule_steps, weight_decay, decoupled, param_groups) -> None:
        """Device state of the schedule path: the rate table, the schedule block (t, scale, lr_now) and (lr multiplier, weight
        decay) per slot; it walks the guarded step's slot table whether or not the step is guarded."""
        from . import schedules as S
        self.lr_table = S.schedule_table(self.lr, lr_schedule, schedule_steps)
        self.weight_decay = float(weight_decay)
        self.decoupled = bool(decoupled)
        self.slot_hp = S.resolve_param_groups(self.names, param_groups, self.weight_decay)
        self._init_slots(dev)
        self._table_dev = torch.tensor(self.lr_table, dtype=torch.float32).to(dev)
        self._hp_dev = torch.tensor(self.slot_hp, dtype=torch.float32).reshape(-1, 2).contiguous().to(dev)
        self.sched_dev = E.sched_state(dev)
        self._sched_views = E.sched_views(self.sched_dev)
        self.last_lr = self._sched_views["lr_now"]

    def _need_hp(self) -> None:
        if not self.hp:
            raise RuntimeError("TrainStep: built without lr_schedule / weight_decay / param_groups, there is no schedule to read")

    def _hp_update(self, scale: float, status: Optional[Tensor] = None) -> None:
        """The rate of this step, then Adam over all slots with it; `status` None: the unguarded step."""
        E.lr_advance(self.sched_dev, self._table_dev, self._mask_dev, self.slot_steps_dev, status)
        E.adam_slots_hp(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self._slots_dev, self._mask_dev,
                        self.slot_steps_dev, self._hp_dev, self.sched_dev, status, self.betas[0], self.betas[1], self.eps,
                        decoupled=self.decoupled, grad_scale=scale)

    def schedule_position(self) -> int:
        """Applied steps the schedule has seen = index of the next table entry (reads the device: host synchronisation)."""
        self._need_hp()
        return int(self._sched_views["t"])

    def set_lr_scale(self, s: float) -> None:
        """Multiply every table entry by `s` from the next step on (reduce-on-plateau: set_lr_scale(0.1 * current)): a
        stream-ordered write into the schedule block, legal between replays, not inside a capture."""
        self._need_hp()
        s = float(s)
        if not (s >= 0.0 and s != float("inf")):
            raise ValueError(f"TrainStep.set_lr_scale: {s!r}, a finite scale >= 0 is needed")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TrainStep.set_lr_scale(): not inside a hipGraph capture (the graph would bake the value in)")
        self._sched_views["scale"].fill_(s)

    def _optim_record(self) -> dict:
        """What a snapshot notes about the schedule path, for diagnosis on load."""
        from . import schedules as S
        return {"table_len": len(self.lr_table), "table_digest": S.table_digest(self.lr_table), "table": list(self.lr_table),
                "groups": {n: [float(a), float(b)] for n, (a, b) in zip(self.names, self.slot_hp)},
                "decoupled": self.decoupled, "weight_decay": self.weight_decay}

    def _set_mask(self, flags: List[bool]) -> None:
        """Upload the mask of trainable slots when the flags have changed (stream-ordered copy; never under capture)."""
        if flags != self._mask_flags:
            _, mask = slot_table(self.offsets, self.total, flags)
            self._mask_dev.copy_(torch.tensor(mask, dtype=torch.int32))
            self._mask_flags = list(flags)

    def _save_buffers(self) -> None:
        if self.flat_buf is not None and self.flat_buf.numel():
            self._buf_saved.copy_(self.flat_buf)

    def _guarded_update(self, scale: float) -> None:
        """norm -> decision -> Adam over all slots -> roll-back of the buffers; the mask is on the device already."""
        E.grad_sumsq(self.flat_grad, self._slots_dev, self._mask_dev, self.ws, self._status)
        E.step_decide(self._status, self.max_grad_norm, scale, self.skip_nonfinite, self._mask_dev, self.slot_steps_dev,
                      self._skip_dev)
        if self.hp:
            self._hp_update(scale, self._status)
        else:
            E.adam_slots(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self._slots_dev, self._mask_dev,
                         self.slot_steps_dev, self._status, self.lr, self.betas[0], self.betas[1], self.eps)
        if self.flat_buf is not None and self.flat_buf.numel():
            E.restore_if_skipped(self.flat_buf, self._buf_saved, self._status)

    def _need_guard(self) -> None:
        if not self.guarded:
            raise RuntimeError("TrainStep: built without max_grad_norm / skip_nonfinite, there is no guarded step to read")

    def skipped_steps(self) -> int:
        """Steps skipped so far because their gradient was not finite (reads a device counter: host synchronisation)."""
        self._need_guard()
        return int(self._skip_dev)

    def sync_steps(self) -> None:
        """Bring the host's `param_steps` / `step_count` in line with the device's counts (host synchronisation): they count
        a skipped step as taken until this is called."""
        self._need_guard()
        self.param_steps = [int(s) for s in self.slot_steps_dev.tolist()]
        self.step_count = self._attempts - int(self._skip_dev)

    # ------------------------------------------------------------------------------------------------
    def trainable_flags(self) -> List[bool]:
        return [p.requires_grad for _, p in self._named]

    def _xruns(self, flags: List[bool]) -> Optional[List[Tuple[int, int]]]:
        """Ranges of the gradient exchange: None = the whole buffer (every parameter trains)."""
        return None if all(flags) else trainable_runs(self.offsets, self.total, flags)

    def _adam_runs(self, flags: List[bool]) -> List[Tuple[int, int, int]]:
        """(start, end, step count) of every Adam launch: runs of trainable slots with one step count."""
        runs = trainable_runs(self.offsets, self.total, flags, self.param_steps)
        first = {}
        for i in range(len(self.offsets) - 1, -1, -1):
            first[self.offsets[i]] = i
        return [(b, e, self.param_steps[first[b]]) for b, e in runs]

    def _forward_backward(self, x: Tensor, dates: Tensor, y: Tensor, drop: Fn.DropoutState, overlap_exchange: bool = False,
                          flags: Optional[List[bool]] = None) -> Tuple[Tensor, Tensor]:
        """zero_grad -> forward -> CE -> backward into the flat gradient buffer (stream-ordered, no host sync).  Frozen slots
        of the buffer (flags False) are not written."""
        model = self.model
        flags = self.trainable_flags() if flags is None else flags
        tape = E.Tape()
        train = None if all(flags) else [n for n, f in zip(self.names, flags) if f]
        grads = self.grads if train is None else {n: self.grads[n] for n in train}
        ctx = E.Ctx(self.params, dict(model.named_buffers()), grads, self.ws, model.training, tape, trainable=train)
        xruns = self._xruns(flags)
        ctx.want_att = False                             # the step returns (loss, logits): nobody reads the attention masks
        self._early, self._early_off = None, 0
        if (overlap_exchange and self.dp is not None and self.dp.active and OVERLAP_EXCHANGE and not E.REDUCE_BATCH
                and not torch.cuda.is_current_stream_capturing()):
            # Gradient exchange in two buckets: the tape runs this hook once the backward pass has left the decoder
            # and the temporal encoder -- everything behind the per-frame encoder in the flat buffer is final then -- and that
            # suffix is summed over the ranks on a communication stream while the encoder's backward pass (the bulk of the
            # step) still runs; the encoder's own gradients follow after the join.
            def early_exchange():
                tape.flush_side()                        # the weight-gradient launches queued so far
                i = early_cut(self.names, ctx._gwritten, flags)   # the suffix of final gradients, frozen slots included
                if i == 0 or i == len(self.names):
                    return
                off = self.offsets[i]
                after = (E._side_stream(),) if tape.side_used else ()
                if xruns is None:
                    self._early_off = off
                    self._early = [self.dp.reduce_async(self.flat_grad[off:], after=after)]
                    return
                runs = clip_runs(xruns, off, self.total)     # only the trainable runs of the suffix
                if runs:
                    self._early_off = off
                    self._early = [self.dp.reduce_async(self.flat_grad[b:e], after=after) for b, e in runs]
            ctx.early_hook = early_exchange
        out = Fn.FORWARDS[model.spec.model](ctx, model.spec, x, dates, drop)
        logits = out.logits
        if self.criterion is None:
            loss, glogits = E.cross_entropy(logits, y, self.class_w, self.ws, want_grad=True, label_smoothing=self.label_smoothing)
        else:
            loss, glogits = self._criterion_loss(logits, y)
        tape.grads[logits.data_ptr()] = glogits
        if out.boundary is not None:
            # src/learning/utils.py:283-285,318-324: y_b from the dilated one-hot labels, loss = CE + FocalCE(out_b, y_b)
            from .losses import boundary_target, focal_ce
            y_b = boundary_target(y)
            _, g_b = focal_ce(out.boundary, y_b, self.boundary_gamma, want_grad=True, ws=self.ws, loss_out=loss)
            tape.grads[out.boundary.data_ptr()] = g_b
            self.last_boundary = out.boundary
        tape.backward()
        if not torch.cuda.is_current_stream_capturing():
            self.ws.finalize_pack_plan()                 # from the second step on, all weight packs are one launch
        for n, f in zip(self.names, flags):              # trainable parameters no kernel wrote to (none in the default models)
            if f and n not in ctx._gwritten:
                self.grads[n].zero_()
        return loss, logits

    def _criterion_loss(self, logits: Tensor, y: Tensor) -> Tuple[Tensor, Tensor]:
        """The main loss from `self.criterion` (iterate(..., criterion=criterion), train.py:466-474,488): the value as a [1]
        view of the criterion's own device scalar -- the boundary head's focal_ce(loss_out=loss) adds onto it -- and
        dL/dlogits from grad().  A criterion that hands back no gradient is an error, never a reason to fall back."""
        value = self.criterion(logits, y, want_grad=True)
        glogits = self.criterion.grad()
        if not torch.is_tensor(value) or value.numel() != 1 or value.device != logits.device or value.dtype != torch.float32:
            raise RuntimeError("TrainStep: criterion(logits, y, want_grad=True) must return one float32 value on the logits' device")
        if glogits is None or glogits.shape != logits.shape or glogits.dtype != torch.float32 or not glogits.is_contiguous():
            raise RuntimeError("TrainStep: criterion.grad() must return a contiguous float32 dL/dlogits of the logits' shape")
        return value.reshape(1), glogits

    def bad_targets(self) -> int:
        """Labels outside [0, num_classes) (other than ignore_index) in the last step's batch: torch's CrossEntropyLoss raises on
        them, the loss kernel skips and counts them -- call this every display_step to surface a mislabelled dataset
        (host synchronisation).  With a criterion that has bad_target_count() the count is the criterion's.  Also the place
        where a failed one-pass normalisation wait surfaces (`check_health`)."""
        if self.criterion is not None and hasattr(self.criterion, "bad_target_count"):
            n = int(self.criterion.bad_target_count())
        else:
            n = E.bad_target_count(self.ws)
        self.check_health()
        return n

    def check_health(self) -> None:
        """Host-synchronising health check (every display_step; `StepMeters.watch(step)` calls it from `get_miou_acc()` /
        `loss_mean()`): raises if a one-pass normalisation wait gave up (engine.Workspace.check_sync: the area is reset and
        the process continues on the two-pass kernels).  A captured graph has the one-pass launches baked in, so it is
        dropped and has to be captured again.  The step that hit the failed wait produced NaN: with skip_nonfinite=True it
        changed nothing (the device skipped it: `skipped_steps()`), so the caller may catch the error and repeat the step; without
        it the NaN has gone through Adam into the parameters, the moments and the BatchNorm running statistics, and the
        way back is the last checkpoint: `TrainStep.load(path)` for a file written by `snapshot().save(path)`, or
        `load_state_dict(snap.state_dict())` for a snapshot kept in memory (capture() again afterwards: the graphs are
        dropped here)."""
        try:
            self.ws.check_sync()
        except RuntimeError:
            self.graph_fb = self.graph_opt = None
            raise

    def _seed_root_value(self) -> int:
        """Root of the dropout seed sequence: torch.initial_seed(), or the root of the state that was loaded."""
        root = getattr(self, "_seed_root", None)
        return torch.initial_seed() if root is None else root

    def _rank(self) -> int:
        return self.dp.rank if self.dp is not None else 0

    @staticmethod
    def _dropout_base(root: int, calls: int, rank: int) -> int:
        return (root * 0x9E3779B1 + calls * 2 + rank * 0x51ED27) & ((1 << 62) - 1)

    def _fresh_dropout(self) -> Fn.DropoutState:
        drop = Fn.DropoutState()
        if self.model.training:
            self._seed_calls = getattr(self, "_seed_calls", 0) + 1
            base = self._dropout_base(self._seed_root_value(), self._seed_calls, self._rank())
            drop.attn_seed, drop.mlp_seed = base, base + 1
        return drop

    @torch.no_grad()
    def __call__(self, x: Tensor, dates: Tensor, y: Tensor, dropout_state: Optional[Fn.DropoutState] = None,
                 apply_update: bool = True) -> Tuple[Tensor, Tensor]:
        """Eager step.  Returns (loss[1] device tensor, logits).  No host synchronisation inside."""
        self.model._check_inputs(x, dates)
        drop = dropout_state if dropout_state is not None else self._fresh_dropout()
        flags = self.trainable_flags()
        if not any(flags):
            raise ValueError("TrainStep: no parameter requires grad")
        if self.guarded and apply_update:
            self._set_mask(flags)
            self._save_buffers()                         # what a skipped step puts back
        elif self.hp and apply_update:
            self._set_mask(flags)
        loss, logits = self._forward_backward(x.contiguous(), dates.contiguous(), y, drop, overlap_exchange=True, flags=flags)
        xruns = self._xruns(flags)
        scale = 1.0
        if self.dp is not None:
            if self._early is not None:                                   # the decoder's bucket has been under way since the
                if xruns is None:                                         # backward pass entered the encoder
                    scale = self.dp.reduce_gradients(self.flat_grad[:self._early_off])
                else:
                    scale = self.dp.reduce_gradients(self.flat_grad, runs=clip_runs(xruns, 0, self._early_off))
                for h in self._early:
                    if h is not None:
                        h.wait()
                self._early = None
            else:
                scale = self.dp.reduce_gradients(self.flat_grad, runs=xruns)     # one 4.3 MB bucket per step
        if apply_update:
            self.step_count += 1
            self.param_steps = [s + 1 if f else s for s, f in zip(self.param_steps, flags)]
            if self.guarded:
                self._attempts += 1
                self._guarded_update(scale)
                return loss, logits
            if self.hp:
                self._hp_update(scale)
                return loss, logits
            for b, e, st in self._adam_runs(flags):
                E.adam_flat(self.flat_param[b:e], self.flat_grad[b:e], self.exp_avg[b:e], self.exp_avg_sq[b:e], st, self.lr,
                            self.betas[0], self.betas[1], self.eps, grad_scale=scale)
        return loss, logits

    # ------------------------------------------------------------------------------------------------
    # hipGraph path: the whole step (about 335 kernel launches, ~3 ms of host time when launched eagerly) is
    # captured once and replayed.  Everything the step needs to vary between replays lives on the device: the
    # dropout seed offset and the Adam step count are device counters advanced inside the graph.
    @torch.no_grad()
    def capture(self, x: Tensor, dates: Tensor, y: Tensor) -> None:
        """Capture the step for inputs of this shape.  `x`, `dates`, `y` are copied into static buffers; call
        `replay(x, dates, y)` (or `replay()` to reuse the buffers' content) afterwards.  The set of parameters that require
        grad is fixed here: replay() raises once it has changed (capture again)."""
        self.model._check_inputs(x, dates)
        dev = x.device
        flags = self.trainable_flags()
        if not any(flags):
            raise ValueError("TrainStep: no parameter requires grad")
        self.static_x, self.static_dates, self.static_y = x.clone().contiguous(), dates.clone().contiguous(), y.clone()
        runs = None
        if self.guarded or self.hp:
            self._set_mask(flags)                       # these steps keep their step counts per slot (slot_steps_dev)
        else:
            runs = self._adam_runs(flags)               # one device step counter per Adam launch
            self.step_dev = torch.tensor([st for _, _, st in runs], device=dev, dtype=torch.int32)
        pending = getattr(self, "_pending_capture", None)
        if pending is not None:
            # a loaded state was saved by a captured step: the graph bakes the dropout base in by value, so the continuation
            # takes the recorded base (its place in the seed sequence) and replay counter instead of drawing a fresh one
            drop = Fn.DropoutState()
            if self.model.training:
                base = self._dropout_base(self._seed_root_value(), pending["calls"], self._rank())
                drop.attn_seed, drop.mlp_seed = base, base + 1
            self.seed_dev = torch.tensor([pending["seed_dev"]], device=dev, dtype=torch.int64)
            self._cap_calls = pending["calls"]
            self._pending_capture = None
        else:
            self.seed_dev = torch.zeros(1, device=dev, dtype=torch.int64)
            drop = self._fresh_dropout()
            self._cap_calls = getattr(self, "_seed_calls", 0)
        self._cap_base = drop.attn_seed
        drop.seed_dev = self.seed_dev
        saved = {k: v.clone() for k, v in self.model.named_buffers()}     # the warm-up pass must not count as a step
        # the captured step runs on one stream: all slice sums of the weight gradients go into ONE launch at its end
        # (engine.REDUCE_BATCH; same order of additions); the warm-up pass below builds the job table the capture reuses
        batch0, E.REDUCE_BATCH = E.REDUCE_BATCH, True
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                   # warm-up on the side stream: lazy one-time initialisation
                self._forward_backward(self.static_x, self.static_dates, self.static_y, drop, flags=flags)   # (function
                                                            # attributes, workspaces)
            torch.cuda.current_stream().wait_stream(side)
            for k, v in self.model.named_buffers():
                v.copy_(saved[k])
            torch.cuda.synchronize()
            self.check_health()                             # never bake a poisoned sync area into a graph
            scale = 1.0 / self.dp.world if self.dp is not None else 1.0
            self.graph_fb = torch.cuda.CUDAGraph()
            # capture_error_mode thread_local: the process group's watchdog thread keeps polling the events of earlier collectives
            # (hipEventQuery), which the default global mode forbids while ANY thread captures
            with torch.cuda.graph(self.graph_fb, capture_error_mode="thread_local"):
                self.seed_dev.add_(1)
                if self.guarded:
                    self._save_buffers()
                self.static_loss, self.static_logits = self._forward_backward(self.static_x, self.static_dates, self.static_y, drop,
                                                                              flags=flags)
        finally:
            E.REDUCE_BATCH = batch0
        self.graph_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_opt, capture_error_mode="thread_local"):
            if self.guarded:                            # after the exchange that sits between the two graphs
                self._guarded_update(scale)
            elif self.hp:                               # the rate and the step counts advance on the device: no step_dev
                self._hp_update(scale)
            else:
                self.step_dev.add_(1)
                for k, (b, e, _) in enumerate(runs):
                    E.adam_flat(self.flat_param[b:e], self.flat_grad[b:e], self.exp_avg[b:e], self.exp_avg_sq[b:e], 0, self.lr,
                                self.betas[0], self.betas[1], self.eps, grad_scale=scale, step_dev=self.step_dev[k:k + 1])
        self._cap_flags = flags
        self._cap_runs = runs

    @torch.no_grad()
    def replay(self, x: Optional[Tensor] = None, dates: Optional[Tensor] = None, y: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        if getattr(self, "graph_fb", None) is None:
            raise RuntimeError("TrainStep.replay(): no captured step (capture() was not called, or check_health() dropped it)")
        flags = self.trainable_flags()
        if flags != self._cap_flags:
            raise RuntimeError("TrainStep.replay(): the set of parameters that require grad has changed since capture(); "
                               "call capture() again")
        if x is not None:
            self.static_x.copy_(x)
            self.static_dates.copy_(dates)
            self.static_y.copy_(y)
        self.graph_fb.replay()
        if self.dp is not None:
            self.dp.reduce_gradients(self.flat_grad, runs=self._xruns(flags))     # between the two graphs, on the same stream
        self.graph_opt.replay()
        self.step_count += 1
        if self.guarded:
            self._attempts += 1
        self.param_steps = [s + 1 if f else s for s, f in zip(self.param_steps, flags)]
        return self.static_loss, self.static_logits

    # ------------------------------------------------------------------------------------------------
    # Snapshots and checkpoints (csrc/snapshot.hip, checkpoint.py; DESIGN.md, checkpoints): the whole training state as one
    # device blob per snapshot, gathered by one launch and copied to the host behind the step.
    def _captured(self) -> bool:
        return getattr(self, "graph_fb", None) is not None

    def release_capture(self) -> None:
        """Drop the captured graphs (before loading a state they do not fit; capture() again afterwards)."""
        self.graph_fb = self.graph_opt = None

    def _snapshot_regions(self) -> List[Tuple[str, Tensor]]:
        """The live device tensors that make up the state, in blob order."""
        flat_buf = getattr(self, "flat_buf", None)
        regs = [("flat_param", self.flat_param), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)]
        if flat_buf is not None:
            regs.append(("flat_buf", flat_buf))             # every floating-point buffer is a view of it
        for k, b in self.model.named_buffers():
            if flat_buf is None or not b.is_floating_point():
                regs.append(("buffer:" + k, b))
        if self.guarded:
            regs += [("slot_steps_dev", self.slot_steps_dev), ("_skip_dev", self._skip_dev)]
        if self.hp:
            if not self.guarded:
                regs.append(("slot_steps_dev", self.slot_steps_dev))
            regs.append(("sched_dev", self.sched_dev))
        if self._captured():
            if not self.guarded and not self.hp:
                regs.append(("step_dev", self.step_dev))
            regs.append(("seed_dev", self.seed_dev))
        return regs

    def _snapshot_plan(self) -> dict:
        """Layout, device table, the two staging blobs and the status block: planned once and kept while the regions stay
        where they are (capture() adds two)."""
        from .. import checkpoint as CK
        regs = self._snapshot_regions()
        key = tuple((n, t.data_ptr(), t.numel() * t.element_size()) for n, t in regs)
        plan = getattr(self, "_snap_plan", None)
        if plan is not None and plan["key"] == key:
            return plan
        for n, t in regs:
            if not t.is_contiguous() or (t.numel() * t.element_size()) % 4:
                raise ValueError(f"TrainStep.snapshot: {n} must be contiguous and a multiple of 4 bytes long")
        dev = self.flat_param.device
        cur = torch.cuda.current_stream()
        if plan is not None:
            for ev in plan["done"]:                         # the old staging blobs go back to the allocator of this stream
                if ev is not None:
                    cur.wait_event(ev)
        nbytes = [k[2] for k in key]
        offs, payload, _ = CK.plan_layout(nbytes)
        flat_buf = getattr(self, "flat_buf", None)
        named_b = list(self.model.named_buffers())
        static = {
            "keys": list(self.model.state_dict().keys()), "names": list(self.names),
            "shapes": [tuple(p.shape) for _, p in self._named], "offsets": list(self.offsets),
            "flat_buf_views": [(k, tuple(b.shape)) for k, b in named_b if flat_buf is not None and b.is_floating_point()],
            "buffers": [(k, tuple(b.shape), b.dtype) for k, b in named_b if flat_buf is None or not b.is_floating_point()],
        }
        total = E.SNAPSHOT_HEADER_BYTES + payload
        plan = self._snap_plan = {
            "key": key, "regions": [(n, nb, o) for (n, _, nb), o in zip(key, offs)], "payload": payload, "n": len(regs),
            "table": E.snapshot_table([k[1] for k in key], nbytes, offs, dev),
            "blobs": [torch.empty(total, device=dev, dtype=torch.uint8) for _ in range(2)], "done": [None, None], "count": 0,
            "status": E.snapshot_status(dev), "stream": plan["stream"] if plan is not None else torch.cuda.Stream(),
            "static": static,
        }
        return plan

    def _staging(self, plan: dict) -> Tuple[int, Tensor]:
        """The staging blob whose turn it is; the current stream waits for the copy that still reads it."""
        k = plan["count"] % 2
        plan["count"] += 1
        if plan["done"][k] is not None:
            torch.cuda.current_stream().wait_event(plan["done"][k])
        return k, plan["blobs"][k]

    @torch.no_grad()
    def snapshot(self):
        """The training state at this point of the current stream, as a checkpoint.Snapshot: one gather launch into one of two
        device staging blobs, then a copy to a pinned host blob on a side stream behind an event.  No host synchronisation:
        the next step may be launched at once; a third snapshot while both staging blobs are in flight makes the stream (not
        the host) wait for the older copy.  The host-side scalars are read now; in a guarded step they may lag the device
        (`sync_steps`), and Snapshot.state_dict() takes the step and skip counts from the blob instead."""
        from .. import checkpoint as CK
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("TrainStep.snapshot(): not inside a hipGraph capture (the copy to the host is not part of a step)")
        plan = self._snapshot_plan()
        k, blob = self._staging(plan)
        cur, side = torch.cuda.current_stream(), plan["stream"]
        E.snapshot_gather(plan["table"], plan["n"], blob)
        ready = torch.cuda.Event()
        ready.record(cur)
        host = torch.empty(blob.numel(), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            host.copy_(blob, non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        plan["done"][k] = done
        meta = dict(plan["static"])
        meta.update(
            param_steps=list(self.param_steps), step_count=self.step_count, attempts=getattr(self, "_attempts", 0),
            seed_calls=getattr(self, "_seed_calls", 0), seed_root=self._seed_root_value(), rank=self._rank(),
            guard={"max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite} if self.guarded else None,
            capture={"calls": self._cap_calls, "base": self._cap_base, "flags": list(self._cap_flags)} if self._captured() else None,
            trainable=dict(zip(self.names, self.trainable_flags())), lr=self.lr, betas=tuple(self.betas), eps=self.eps)
        if self.hp:
            meta["optim"] = self._optim_record()
        return CK.Snapshot(host, done, plan["regions"], meta)

    def _check_state(self, state: dict, exact: bool) -> None:
        """ValueError listing every difference in names, shapes or guard mode between `state` and this step."""
        from .. import checkpoint as CK
        diffs = []
        if not isinstance(state, dict) or "state_dict" not in state:
            raise ValueError("TrainStep.load_state_dict: a dict with a 'state_dict' entry is needed")
        extra = state.get(CK.EXTRA_KEY)
        if extra is not None and not exact:
            raise ValueError(f"TrainStep.load_state_dict: '{CK.EXTRA_KEY}' has layout version "
                             f"{extra.get('layout_version') if isinstance(extra, dict) else extra!r}, this build reads {CK.LAYOUT_VERSION}")
        sd = state["state_dict"]
        mine = self.model.state_dict()
        for k, v in mine.items():
            if k not in sd:
                diffs.append(f"{k}: missing in the state")
            elif tuple(sd[k].shape) != tuple(v.shape):
                diffs.append(f"{k}: shape {tuple(sd[k].shape)} in the state, {tuple(v.shape)} in the model")
        diffs += [f"{k}: not in the model" for k in sd if k not in mine]
        if exact:
            g = extra["guard"]
            theirs = (g is not None, bool(g["skip_nonfinite"]) if g is not None else False)
            if theirs != (self.guarded, self.skip_nonfinite):
                diffs.append(f"guard mode: the state has (guarded, skip_nonfinite) = {theirs}, this step "
                             f"{(self.guarded, self.skip_nonfinite)}")
            if extra.get("optim") is not None and not self.hp:
                diffs.append("schedule mode: the state was written with lr_schedule / weight_decay / param_groups (its step "
                             "counts and schedule position live on the device), this step was built without them")
            if len(extra["param_steps"]) != len(self.names):
                diffs.append(f"step counts: {len(extra['param_steps'])} in the state, {len(self.names)} parameters")
        if diffs:
            raise ValueError("TrainStep.load_state_dict: the state does not fit this step; nothing was loaded:\n  " + "\n  ".join(diffs))

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> dict:
        """Put a state of Snapshot.state_dict() / TrainStep.load() back, in place: one blob is uploaded, verified on the device
        and scattered into the live tensors, so parameters stay views of `flat_param`, buffers of `flat_buf`, and a captured
        graph stays valid.  Then the host-side scalars follow (step counts, seed root and call count, the trainable flags by
        name).  lr / betas / eps stay the constructor's.  One host synchronisation (the verdict is read back).

        ValueError (with the list of differences) when names, shapes or guard mode differ; RuntimeError when the device refused
        the blob (its sums do not match the state's record) or when a captured step is given a state that does not carry its
        dropout base.  In all three cases nothing has been written.  A state with only the reference's keys loads parameters,
        buffers, moments and step counts; the return value's "bit_exact" is False then, and a warning says so.

        On the schedule path the schedule block comes back from the state's own words; the table, the groups and
        the decay stay the constructor's, and the return value says where the state's record differs ("optim_differs":
        {"schedule", "groups", "mode"}).  A state written without the path starts the schedule at its applied step count with
        scale 1 ("optim_differs" None; "schedule_bit_exact" False if its per-slot counts are unequal).  A state written with the
        path does not fit a step built without it (ValueError)."""
        from .. import checkpoint as CK
        import numpy as np
        exact = CK.is_bit_exact(state)
        self._check_state(state, exact)
        extra = state[CK.EXTRA_KEY] if exact else None
        shapes = [tuple(p.shape) for _, p in self._named]
        flat_p, flat_m, flat_v, steps, bufs = CK.torch_to_flat(state, self.names, shapes, self.offsets, self.total)
        if exact:
            steps = [int(s) for s in extra["param_steps"]]
            bufs.update(extra.get("extra_buffers", {}))
        cap = extra.get("capture") if exact else None
        values: Dict[str, Tensor] = {}
        if self._captured():
            fits = cap is not None and list(cap["flags"]) == list(self._cap_flags) and \
                self._dropout_base(extra["seed_root"], cap["calls"], self._rank()) == self._cap_base
            if fits and not self.guarded and not self.hp:
                first = {o: i for i, o in reversed(list(enumerate(self.offsets)))}
                ends = list(self.offsets[1:]) + [self.total]
                for b, e, _ in self._cap_runs:
                    run = {steps[i] for i, o in enumerate(self.offsets) if b <= o < e and ends[i] > o}
                    fits = fits and len(run) <= 1
                values["step_dev"] = torch.tensor([steps[first[b]] for b, _, _ in self._cap_runs], dtype=torch.int32)
            if not fits:
                raise RuntimeError("TrainStep.load_state_dict: the captured graphs have their dropout base and parameter runs baked "
                                   "in and this state does not carry them; nothing was loaded.  Call release_capture(), load, "
                                   "then capture() again")
            values["seed_dev"] = torch.tensor([cap["seed_dev"]], dtype=torch.int64)
        plan = self._snapshot_plan()
        st = plan["static"]
        values.update(flat_param=flat_p, exp_avg=flat_m, exp_avg_sq=flat_v)
        if st["flat_buf_views"] or getattr(self, "flat_buf", None) is not None:
            fb = torch.zeros(self.flat_buf.numel(), dtype=torch.float32)
            o = 0
            for k, shp in st["flat_buf_views"]:
                n = bufs[k].numel()
                fb[o:o + n] = bufs[k].to(torch.float32).reshape(-1)
                o += (n + 3) // 4 * 4
            values["flat_buf"] = fb
        for k, shp, dt in st["buffers"]:
            if k not in bufs:
                raise ValueError(f"TrainStep.load_state_dict: buffer {k} is not in the state; nothing was loaded")
            values["buffer:" + k] = bufs[k].to(dt).reshape(shp)
        if self.guarded:
            values["slot_steps_dev"] = torch.tensor(steps, dtype=torch.int32)
            values["_skip_dev"] = torch.tensor([extra["guard"]["skipped"] if exact else 0], dtype=torch.int32)
        report = {}
        if self.hp:
            theirs = extra.get("optim") if exact else None
            values["slot_steps_dev"] = torch.tensor(steps, dtype=torch.int32)
            if theirs is not None:                      # t and scale as the device held them
                values["sched_dev"] = torch.tensor([int(w) for w in theirs["sched_words"]], dtype=torch.int32)
                mine = self._optim_record()
                report["optim_differs"] = {
                    "schedule": (theirs["table_len"], theirs["table_digest"]) != (mine["table_len"], mine["table_digest"]),
                    "groups": {k: list(v) for k, v in theirs["groups"].items()} != mine["groups"],
                    "mode": (bool(theirs["decoupled"]), float(theirs["weight_decay"])) != (mine["decoupled"], mine["weight_decay"])}
                report["schedule_bit_exact"] = True
            else:                                       # a state from a step without a schedule: t = its applied steps, scale 1
                t0 = int(extra["step_count"]) if exact else (max(steps) if steps else 0)
                values["sched_dev"] = E.sched_state("cpu", t0, 1.0)
                report["optim_differs"] = None
                report["schedule_bit_exact"] = len(set(steps)) <= 1     # unequal counts: no single position fits them all
        # the blob, in this step's layout; its header carries the sums the state recorded, region by region
        host = torch.zeros(E.SNAPSHOT_HEADER_BYTES + plan["payload"], dtype=torch.uint8, pin_memory=True)
        arr = host.numpy()
        recorded = {n: (nb, a, b) for n, nb, a, b in extra["regions"]} if exact else {}
        parts = []
        for n, nb, off in plan["regions"]:
            raw = values[n].contiguous().numpy().reshape(-1).view(np.uint8)
            if raw.size != nb:
                raise ValueError(f"TrainStep.load_state_dict: {n} has {raw.size} bytes in the state, {nb} in this step; nothing was loaded")
            a0 = E.SNAPSHOT_HEADER_BYTES + off
            arr[a0:a0 + nb] = raw
            if n in recorded and recorded[n][0] == nb:
                parts.append((off, recorded[n][1], recorded[n][2]))
            else:
                parts.append((off,) + CK.word_sums(arr[a0:a0 + nb]))
        s1, s2 = CK.compose_sums(parts)
        arr[:E.SNAPSHOT_HEADER_BYTES] = np.frombuffer(CK.blob_header(plan["n"], plan["payload"], s1, s2), dtype=np.uint8)
        _, blob = self._staging(plan)
        blob.copy_(host, non_blocking=True)
        E.snapshot_verify(blob, plan["n"], plan["status"])
        E.snapshot_scatter(plan["table"], plan["n"], blob, plan["status"])
        ok, reason = (int(v) for v in plan["status"].view(torch.int32)[:2].tolist())       # load is a host-side operation
        if ok != 1:
            why = {1: "magic", 2: "version", 3: "region count", 4: "payload size", 5: "checksum"}.get(reason, str(reason))
            raise RuntimeError(f"TrainStep.load_state_dict: the device refused the blob ({why} mismatch: the state's tensors are not "
                               "the ones its checksums were taken from); the live state is untouched")
        self.param_steps = list(steps)
        if exact:
            self.step_count = int(extra["step_count"])
            self._seed_calls, self._seed_root = int(extra["seed_calls"]), int(extra["seed_root"])
            if self.guarded:
                self._attempts = int(extra["guard"]["attempts"])
            for n, p in self._named:
                if n in extra["trainable"]:
                    p.requires_grad_(bool(extra["trainable"][n]))
        else:
            self.step_count = max(steps) if steps else 0
            if self.guarded:
                self._attempts = self.step_count
            CK.warn_not_bit_exact()
        if not self._captured():
            self._pending_capture = None if cap is None else {"calls": int(cap["calls"]), "seed_dev": int(cap["seed_dev"])}
        return dict({"bit_exact": exact, "epoch": state.get("epoch"), "best_mIoU": state.get("best_mIoU")}, **report)

    def load(self, path) -> dict:
        """load_state_dict of a file written by Snapshot.save() -- or by the reference's train.py (model.pth.tar)."""
        return self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
