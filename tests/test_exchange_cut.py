"""Where the two-bucket gradient exchange cuts the flat gradient buffer (`learning.utils.early_cut`) and how `clip_runs` splits
the trainable runs at that cut, on the real parameter names and slot layout of the three models.  No GPU: `TrainStep` only
lays out its flat buffers here.  The written-sets follow the hook positions in backbones/functional.py
(tests/exchange_cases.py); tests/test_exchange_gpu.py checks that the tape really produces them."""
import random

import numpy as np
import pytest
import torch

import exchange_cases as X
from crop2seg_amd.learning.utils import TrainStep, clip_runs, early_cut, trainable_runs


@pytest.fixture(scope="module")
def layouts():
    cache = {}

    def get(model):
        if model not in cache:
            torch.manual_seed(0)
            net = X.model_class(model)(input_dim=10, out_conv=[32, 15])
            sizes = [p.numel() for p in net.parameters()]
            step = TrainStep(net, num_classes=15)
            assert step.names == [n for n, _ in net.named_parameters()]
            cache[model] = (step.names, sizes, step.offsets, step.total)
        return cache[model]
    return get


def _first(names, prefix):
    return next(i for i, n in enumerate(names) if n.startswith(prefix))


def _mask(sizes, offsets, total, flags):
    """Elements of the flat buffer that belong to a trainable slot (its alignment padding included), from the layout alone."""
    m = np.zeros(total, dtype=np.int32)
    ends = offsets[1:] + [total]
    for s, b, e, f in zip(sizes, offsets, ends, flags):
        assert b % 4 == 0 and 0 <= e - b - s < 4          # 16-byte aligned slots, nothing between them but padding
        if f:
            m[b:e] = 1
    return m


def _cover(runs, total):
    c = np.zeros(total, dtype=np.int32)
    for b, e in runs:
        assert 0 <= b < e <= total
        c[b:e] += 1
    return c


@pytest.mark.parametrize("model", X.MODELS)
def test_block_order_matches_the_hook_table(layouts, model):
    """The unwritten blocks are a prefix of named_parameters() and the first early block follows them directly."""
    names = layouts(model)[0]
    k = _first(names, X.FIRST_EARLY[model])
    assert k > 0 and all(n.startswith(X.UNWRITTEN[model]) for n in names[:k])
    assert not any(n.startswith(X.UNWRITTEN[model]) for n in names[k:])
    assert [n.split(".")[0] for n in names[k:]].count("temporal_encoder") > 0 and names[-1].startswith("out_conv.")


@pytest.mark.parametrize("model", X.MODELS)
def test_expected_cut_with_every_parameter_trainable(layouts, model):
    names, sizes, offsets, total = layouts(model)
    flags = X.flags_for(model, names, "all")
    cut = early_cut(names, X.written_at_hook(model, names, flags), flags)
    assert cut == _first(names, X.FIRST_EARLY[model])
    assert 0 < offsets[cut] < total
    assert offsets[cut] == sum((s + 3) // 4 * 4 for s in sizes[:cut])


@pytest.mark.parametrize("model", X.MODELS)
@pytest.mark.parametrize("pattern", X.PATTERNS)
def test_the_two_halves_partition_the_trainable_runs(layouts, model, pattern):
    names, sizes, offsets, total = layouts(model)
    flags = X.flags_for(model, names, pattern)
    cut = early_cut(names, X.written_at_hook(model, names, flags), flags)
    xruns = trainable_runs(offsets, total, flags)
    want = _mask(sizes, offsets, total, flags)
    assert np.array_equal(_cover(xruns, total), want)
    if pattern == "all":
        assert xruns == [(0, total)]
    if cut in (0, len(names)):                               # no early bucket: TrainStep sums `xruns` as they are
        assert pattern == "encoder" and cut == 0
        return
    off = offsets[cut]
    lo, hi = clip_runs(xruns, 0, off), clip_runs(xruns, off, total)
    assert all(e <= off for _, e in lo) and all(b >= off for b, _ in hi)
    assert np.array_equal(_cover(lo, total) + _cover(hi, total), want)      # disjoint (no element twice) and nothing missing
    assert hi, "an early bucket without a trainable run"
    if pattern == "all":
        assert lo == [(0, off)] and hi == [(off, total)]
    if pattern == "te":                                      # the hole splits the suffix in two, the cut stays where it was
        assert cut == _first(names, X.FIRST_EARLY[model]) and len(hi) == 2 and len(lo) == 1


def test_clip_runs_splits_a_run_that_straddles_the_cut():
    runs = [(0, 8), (12, 40), (44, 48)]
    assert clip_runs(runs, 0, 20) == [(0, 8), (12, 20)]
    assert clip_runs(runs, 20, 48) == [(20, 40), (44, 48)]
    assert clip_runs(runs, 8, 12) == [] and clip_runs(runs, 40, 44) == []
    assert clip_runs(runs, 0, 12) == [(0, 8)] and clip_runs(runs, 12, 48) == [(12, 40), (44, 48)]


@pytest.mark.parametrize("model", X.MODELS)
def test_no_early_bucket(layouts, model):
    names = layouts(model)[0]
    flags = X.flags_for(model, names, "encoder")             # the prefix is frozen: the walk runs through to the front
    assert early_cut(names, X.written_at_hook(model, names, flags), flags) == 0
    flags = X.flags_for(model, names, "all")
    assert early_cut(names, set(), flags) == len(names)      # nothing written yet
    assert early_cut(names, set(names), flags) == 0          # everything written: nothing left to overlap with


@pytest.mark.parametrize("model", X.MODELS)
def test_frozen_slots_pass_and_unwritten_trainable_slots_stop_the_walk(layouts, model):
    names = layouts(model)[0]
    k = _first(names, X.FIRST_EARLY[model])
    te = _first(names, "temporal_encoder.")
    # frozen slot inside the suffix
    flags = X.flags_for(model, names, "te")
    written = X.written_at_hook(model, names, flags)
    assert not any(n.startswith("temporal_encoder.") for n in written)
    assert early_cut(names, written, flags) == k
    flags = X.flags_for(model, names, "head+up0")
    assert early_cut(names, X.written_at_hook(model, names, flags), flags) == k
    # the same slot trainable and not written: the suffix starts behind it
    flags = X.flags_for(model, names, "all")
    written = X.written_at_hook(model, names, flags) - {names[te]}
    assert early_cut(names, written, flags) == te + 1
    written = X.written_at_hook(model, names, flags) - {names[-1]}
    assert early_cut(names, written, flags) == len(names)
    # a frozen slot directly in front of the suffix is swallowed (it is never exchanged), a trainable one is not
    flags[k - 1] = False
    assert early_cut(names, X.written_at_hook(model, names, flags), flags) == k - 1
    flags[k - 1], flags[k] = True, False
    assert early_cut(names, X.written_at_hook(model, names, flags), flags) == k


@pytest.mark.parametrize("model", X.MODELS)
def test_a_written_name_in_front_of_an_unwritten_one_stays_outside(layouts, model):
    names = layouts(model)[0]
    k = _first(names, X.FIRST_EARLY[model])
    flags = X.flags_for(model, names, "all")
    written = X.written_at_hook(model, names, flags) | {names[0], names[k - 2]}
    assert early_cut(names, written, flags) == k
    # the defining property, over random written-sets and flags: everything from the cut on is final, and the slot in front
    # of the cut is trainable and unwritten -- so no written name in front of it can be inside
    rng = random.Random(model)
    for trial in range(200):
        p_w, p_f = rng.choice((0.5, 0.9, 0.99)), rng.choice((0.0, 0.1, 0.5))
        flags = [rng.random() >= p_f for _ in names]
        written = {n for n, f in zip(names, flags) if f and rng.random() < p_w}
        cut = early_cut(names, written, flags)
        assert 0 <= cut <= len(names)
        assert all(n in written or not f for n, f in zip(names[cut:], flags[cut:]))
        assert cut == 0 or (flags[cut - 1] and names[cut - 1] not in written)
