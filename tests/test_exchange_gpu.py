"""The two-bucket gradient exchange of `TrainStep` at a simulated world size of 2, against an exact reference.

One process, no process group.  `step.dp` is a real `FlatDataParallel` (world 2, rank 0) whose stream code and loops run as
they are; only `torch.distributed.all_reduce` is replaced by a stand-in that adds the other rank's gradient `g_other` to the
view it is handed, on the stream it is called on, and logs (start, end, stream).  The other rank's gradient is the flat
gradient of a plain step on shard B, this rank's the one of a plain step on shard A (the step is bit-reproducible), so after
the exchanged step on A every trainable slot must hold the single fp32 sum gA + gB bit for bit: a cut that is one slot early,
a slot summed twice or not at all, a gradient written into the early bucket after its collective started all change bits.
Frozen slots hold a sentinel before the step, and `g_other` is 1.0 there, so a collective that touches one is seen.  There is
no tolerance in this file.

The rows can fail.  Observed on an MI355X with three local edits of learning/utils.py that are not part of the project (22
rows: all-train 3, frozen sets 12, optimiser step 3, overlap off 3, captured 1):

(a) `early_cut` returns one slot less, which pulls the last, not yet written encoder parameter into the early bucket:
    16 rows fail.  All-train x3, and frozen "te" and "head+up0" x3 each: the bucket no longer starts at the block the hook
    table names.  Frozen "alternate" x3 and the optimiser step x3: exactly one slot differs from gA + gB, the parameter in
    front of the cut (down_blocks.2.conv2.conv.1.weight, in_conv.conv.conv.4.weight, spatial_reduction.2.conv2.conv.1.weight
    for U-TAE, TimeUNet, W-TAE) -- its weight gradient overwrote the sum.  The captured row fails with the eager optimiser
    step it is compared with.  Still green: frozen "encoder" x3 (no early bucket) and overlap off x3 (the cut is not used).
(b) the prefix collective in `__call__` runs over `[:_early_off + 4]`, so one slot's first four floats are summed twice:
    7 rows fail.  All-train x3 on the logged ranges ((0, off + 4) instead of (0, off)), the optimiser step x3 on the bits of
    `flat_grad`, the captured row through the eager step.  The frozen sets stay green: that line serves only the step in which
    every parameter trains.
(c) `early_exchange` without `tape.flush_side()` and with `after=()` (a race; run once): 15 rows fail.  The early collective
    ran on the communication stream although the tape had forked to the side stream, which the stream check of the all-train
    and the frozen rows with an early bucket (12) reports whatever the data did.  In the optimiser step, which checks data
    only, the bits of `flat_grad` were wrong for U-TAE and W-TAE and right for TimeUNet in that one run; the captured row
    failed with U-TAE's eager step.
tests/test_dist_gpu.py (world size 1, where the sum is the identity) stayed green under (a) and under (b).
"""
import pytest
import torch

import exchange_cases as X

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5
_REF = {}            # (model, pattern) -> (gA, gB): flat gradients of plain steps on the two shards
_EAGER = {}          # model -> Run of the exchanged eager optimiser step (shared with the captured row)


def _shards():
    from oracle import seeded
    a = seeded.make_inputs(2, 4, 10, 32, 32, 91, [4, 3])               # every model's _check_inputs accepts 32 x 32
    b = seeded.make_inputs(2, 4, 10, 32, 32, 57, [3, 4])
    return tuple(t.cuda() for t in a), tuple(t.cuda() for t in b)


def _step(model, pattern):
    from crop2seg_amd.learning.utils import TrainStep
    from oracle import seeded
    torch.manual_seed(0)
    net = X.model_class(model)(input_dim=10, out_conv=[32, 15])
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    net = net.cuda().train()
    net.spec.attn_dropout = 0.0
    net.spec.mlp_dropout = 0.0
    step = TrainStep(net, num_classes=15)
    flags = X.flags_for(model, step.names, pattern)
    for p, f in zip(net.parameters(), flags):
        p.requires_grad_(f)
    assert step.trainable_flags() == flags
    return step, flags


def _slots(step):
    """(name, start, end of the data, end of the slot) of every parameter in the flat buffers."""
    ends = step.offsets[1:] + [step.total]
    return [(n, b, b + p.numel(), e) for (n, p), b, e in zip(step._named, step.offsets, ends)]


def _fill_frozen(step, flags, buf, value):
    for (_, b, _, e), f in zip(_slots(step), flags):
        if not f:
            buf[b:e].fill_(value)


def _reference(model, pattern):
    """gA and gB from plain steps under the same flags, computed once per (model, pattern) and never modified."""
    if (model, pattern) not in _REF:
        from crop2seg_amd.backbones.functional import DropoutState
        step, _ = _step(model, pattern)
        out = []
        for x, dates, y in _shards():
            step(x, dates, y, dropout_state=DropoutState(), apply_update=False)
            out.append(step.flat_grad.clone())
        torch.cuda.synchronize()
        assert not torch.equal(out[0], out[1]) and bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
        _REF[(model, pattern)] = tuple(out)
    return _REF[(model, pattern)]


class Run:
    """One exchanged step (or capture + replay) on shard A with the summing stand-in installed."""

    def __init__(self, model, pattern, apply_update=False, overlap=True, captured=False):
        from crop2seg_amd import engine as E
        from crop2seg_amd.backbones.functional import DropoutState
        from crop2seg_amd.learning import ddp, utils as U
        gA, gB = _reference(model, pattern)
        self.step, self.flags = step, flags = _step(model, pattern)
        self.g_other = g_other = gB.clone()
        _fill_frozen(step, flags, g_other, 1.0)                  # a collective over a frozen slot would move the sentinel
        _fill_frozen(step, flags, step.flat_grad, SENTINEL)
        self.p0 = step.flat_param.clone()
        dp = object.__new__(ddp.FlatDataParallel)
        dp.group, dp.world, dp.rank = None, 2, 0
        assert dp.active
        step.dp = self.dp = dp
        self.log = log = []                                      # (start, end, stream, forks of the tape so far)
        forks = [0]
        fork0 = E.Tape.fork

        def fork(tape):
            forks[0] += 1
            return fork0(tape)

        def all_reduce(t, op=None, group=None, async_op=False):
            fg = step.flat_grad
            assert t.untyped_storage().data_ptr() == fg.untyped_storage().data_ptr(), "not a view of flat_grad"
            assert fg.storage_offset() == 0 and t.is_contiguous() and t.dtype == torch.float32
            assert op == ddp.dist.ReduceOp.SUM and group is None and not async_op
            off, n = t.storage_offset(), t.numel()
            assert n > 0 and off + n <= fg.numel()
            t.add_(g_other[off:off + n])                         # on the current stream, like the collective it stands for
            log.append((off, off + n, torch.cuda.current_stream(), forks[0]))

        (x, dates, y), _ = _shards()
        self.caller = torch.cuda.current_stream()
        torch.cuda.synchronize()
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ddp.dist, "all_reduce", all_reduce)
            mp.setattr(E.Tape, "fork", fork)
            if not overlap:
                mp.setattr(U, "OVERLAP_EXCHANGE", False)
            if captured:
                step.capture(x, dates, y)
                assert log == [], "capture() ran a collective"
                step.replay()
            else:
                step(x, dates, y, dropout_state=DropoutState(), apply_update=apply_update)
            self.early_off = step._early_off
            assert step._early is None
            torch.cuda.synchronize()
        self.ranges = [(b, e) for b, e, _, _ in log]

    def check_gradients(self, gA, gB):
        """Trainable slots hold the one fp32 sum gA + gB, frozen slots (their padding included) the sentinel."""
        want = torch.add(gA, gB)
        got = self.step.flat_grad
        bad = []
        for (n, b, d, e), f in zip(_slots(self.step), self.flags):
            if f and not torch.equal(got[b:d], want[b:d]):
                bad.append(n)
            if not f and not bool((got[b:e] == SENTINEL).all()):
                bad.append("frozen " + n)
        assert not bad, f"{len(bad)} slots differ from gA + gB: {bad[:6]}"
        assert float(want.abs().sum()) > 0

    def check_ranges(self):
        """The logged ranges are pairwise disjoint and their union is exactly the trainable runs."""
        from crop2seg_amd.learning.utils import trainable_runs
        merged = []
        for b, e in sorted(self.ranges):
            assert b < e and (not merged or b >= merged[-1][1]), f"overlapping collectives around {b}"
            if merged and merged[-1][1] == b:                     # slots are contiguous: a run cut in two by the bucket boundary
                merged[-1][1] = e
            else:
                merged.append([b, e])
        assert [tuple(r) for r in merged] == trainable_runs(self.step.offsets, self.step.total, self.flags)

    def check_streams(self):
        """Early collectives (at or behind the cut) ran off the caller's stream -- on the weight-gradient side stream when the
        tape had forked to it, else on the communication stream -- and before the others, which ran on the caller's stream."""
        from crop2seg_amd import engine as E
        early = [r for r in self.log if self.early_off and r[0] >= self.early_off]
        assert self.log[:len(early)] == early, "an early collective was issued after a late one"
        for b, e, stream, forks in early:
            assert stream != self.caller, (b, e)
            assert stream == (E._side_stream() if forks else self.dp._comm), (b, e, forks)
        for b, e, stream, _ in self.log[len(early):]:
            assert stream == self.caller and (not self.early_off or e <= self.early_off), (b, e)
        return early


def _expected_off(run, model):
    from crop2seg_amd.learning.utils import early_cut
    names = run.step.names
    cut = early_cut(names, X.written_at_hook(model, names, run.flags), run.flags)
    return cut, (run.step.offsets[cut] if 0 < cut < len(names) else 0)


@pytest.mark.parametrize("model", X.MODELS)
def test_all_parameters_train(model):
    gA, gB = _reference(model, "all")
    run = Run(model, "all")
    step = run.step
    cut, off = _expected_off(run, model)
    assert run.early_off == off > 0
    assert step.names[cut].startswith(X.FIRST_EARLY[model]) and not step.names[cut - 1].startswith(X.FIRST_EARLY[model])
    assert run.ranges == [(off, step.total), (0, off)]
    assert len(run.check_streams()) == 1
    run.check_gradients(gA, gB)
    assert torch.equal(step.flat_grad, torch.add(gA, gB))        # the alignment padding between the slots as well
    assert torch.equal(step.flat_param, run.p0)                  # apply_update=False


@pytest.mark.parametrize("model", X.MODELS)
@pytest.mark.parametrize("pattern", [p for p in X.PATTERNS if p != "all"])
def test_frozen_sets(model, pattern):
    from crop2seg_amd.learning.utils import trainable_runs
    gA, gB = _reference(model, pattern)
    run = Run(model, pattern)
    step = run.step
    cut, off = _expected_off(run, model)
    assert run.early_off == off
    early = run.check_streams()
    if pattern == "encoder":                                     # nothing left to overlap with: no early bucket
        assert off == 0 and early == []
        assert run.ranges == trainable_runs(step.offsets, step.total, run.flags)
    else:
        assert off > 0 and early
    if pattern in ("te", "head+up0"):                            # frozen slots inside the suffix do not move the cut
        assert step.names[cut].startswith(X.FIRST_EARLY[model]) and not step.names[cut - 1].startswith(X.FIRST_EARLY[model])
    if pattern == "te":
        assert len(early) == 2                                   # the suffix either side of the hole
    run.check_ranges()
    run.check_gradients(gA, gB)


@pytest.mark.parametrize("model", X.MODELS)
def test_one_optimiser_step_applies_half_the_sum(model):
    """The 1/world factor is folded into Adam: parameters and moments against a direct `adam_flat` on gA + gB, scale 0.5."""
    from crop2seg_amd import engine as E
    gA, gB = _reference(model, "all")
    run = _EAGER[model] = Run(model, "all", apply_update=True)
    step = run.step
    gsum = torch.add(gA, gB)
    assert torch.equal(step.flat_grad, gsum)
    p, m, v = run.p0.clone(), torch.zeros_like(run.p0), torch.zeros_like(run.p0)
    E.adam_flat(p, gsum, m, v, 1, step.lr, step.betas[0], step.betas[1], step.eps, grad_scale=0.5)
    torch.cuda.synchronize()
    assert not torch.equal(p, run.p0)
    assert torch.equal(step.flat_param, p) and torch.equal(step.exp_avg, m) and torch.equal(step.exp_avg_sq, v)
    assert step.param_steps == [1] * len(step.names)


@pytest.mark.parametrize("model", X.MODELS)
def test_overlap_off_is_one_collective_with_the_same_bits(model):
    gA, gB = _reference(model, "all")
    run = Run(model, "all", overlap=False)
    assert run.early_off == 0
    assert run.ranges == [(0, run.step.total)] and run.log[0][2] == run.caller
    run.check_gradients(gA, gB)
    assert torch.equal(run.step.flat_grad, torch.add(gA, gB))    # what test_all_parameters_train holds the overlapped step to


def test_captured_step_exchanges_between_its_two_graphs():
    gA, gB = _reference("utae", "all")
    eager = _EAGER.get("utae") or Run("utae", "all", apply_update=True)
    run = Run("utae", "all", captured=True)
    step = run.step
    assert run.ranges == [(0, step.total)] and run.log[0][2] == run.caller
    run.check_gradients(gA, gB)                                  # summed after the first graph ...
    assert torch.equal(step.flat_param, eager.step.flat_param)   # ... and before the second one
    assert not torch.equal(step.flat_param, run.p0)
    assert torch.equal(step.exp_avg, eager.step.exp_avg) and torch.equal(step.exp_avg_sq, eager.step.exp_avg_sq)
