"""The stand-in aggregator of tests/rect_ref.py against the unwrapped oracle (CPU only).

test_models_rect_gpu.py holds U-TAE on wide inputs (W >= 2H) against the oracle with `aggregate_bilinear_either` patched in,
because the reference's att_group aggregator raises there.  That is only a reference if the stand-in IS the oracle wherever
the oracle is defined: here, bit for bit, logits and attention, at 64 x 16, 32 x 56 and 16 x 16, in eval and train mode.
The second test pins the finding itself: on 16 x 64 and 16 x 32 the unwrapped oracle raises and the stand-in returns finite
numbers of the right shape."""
import pytest
import torch

import rect_ref as RR


def _forward(sd, x, dates, training):
    from oracle import crop2seg_oracle as O
    return O.forward(sd, x, dates, O.BackboneConfig(model="utae"), training=training, bn=O.BNState())


def _inputs(H, W):
    from oracle import seeded
    return seeded.make_inputs(2, 4, 10, H, W, 7, [4, 3])


@pytest.fixture(scope="module")
def utae_state():
    return RR.state("utae")


@pytest.mark.parametrize("H,W", [(64, 16), (32, 56), (16, 16)])
@pytest.mark.parametrize("training", [False, True])
def test_stand_in_equals_the_oracle_where_the_reference_is_defined(monkeypatch, utae_state, H, W, training):
    from oracle import crop2seg_oracle as O
    x, dates, _ = _inputs(H, W)
    assert O.temporal_aggregate is RR.ORACLE_AGGREGATE
    logits, att = _forward(utae_state, x, dates, training)
    monkeypatch.setattr(O, "temporal_aggregate", RR.aggregate_bilinear_either)
    logits_s, att_s = _forward(utae_state, x, dates, training)
    assert logits.shape == (2, 15, H, W) and att.shape == (16, 2, 4, H // 8, W // 8)
    assert torch.equal(logits, logits_s) and torch.equal(att, att_s)


@pytest.mark.parametrize("H,W", [(16, 64), (16, 32)])
def test_reference_aggregator_raises_on_wide_inputs_and_the_stand_in_does_not(monkeypatch, utae_state, H, W):
    from oracle import crop2seg_oracle as O
    assert RR.outside_reference_domain("utae", H, W)
    x, dates, _ = _inputs(H, W)
    with pytest.raises(RuntimeError, match="shape .* is invalid for input of size"):
        _forward(utae_state, x, dates, False)
    monkeypatch.setattr(O, "temporal_aggregate", RR.aggregate_bilinear_either)
    logits, att = _forward(utae_state, x, dates, False)
    assert logits.shape == (2, 15, H, W) and att.shape == (16, 2, 4, H // 8, W // 8)
    assert bool(torch.isfinite(logits).all())
