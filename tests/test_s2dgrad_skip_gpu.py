"""The aggregator's input gradient as a pending term of the tape (engine.AGG_SKIP_TERM): temporal_aggregate's backward
stores the interpolated attention weights (c2s_temporal_aggregate_bwd_skip) and the F(2x2,2x2) data gradient of the 4x4
stride-2 convolution that reads the same feature map adds up(attn) * d skip in its epilogue
(c2s_conv4x4s2_dgrad_winograd_skip), against the two-step path of the same library (C2S_AGG_SKIP_TERM=0: the aggregator
writes the products, the data gradient reads, adds and stores).  The product is rounded on its own in both, so the input
gradient is compared bit for bit, padded frames included; each case also asserts which path it took.  Where the fused
kernel does not apply (two channels per head) or something else touches the gradient while the term is pending, the
result must still have the bits of the two-step path.  Last, one train step of a small U-TAE with the switch on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32)


class CountingLib:
    """engine.lib() stand-in that counts the calls of every export and forwards them."""

    def __init__(self, real):
        self.real, self.count = real, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.count[name] = self.count.get(name, 0) + 1
            return fn(*args)
        return call


def run(monkeypatch, fused, B, T, Kc, Ho, Wo, Cs, nh, ratio, reflect=True, pad=(), second=False):
    """x [B T, Cs, 2 Ho, 2 Wo] feeds a 4x4 stride-2 convolution (Kc output channels) and, as [B,T,...], the temporal
    aggregation with attention maps `ratio` times smaller; backward from seeded gradients of both outputs.  Returns the
    gradient of x and the call counts."""
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    monkeypatch.setattr(E, "AGG_SKIP_TERM", fused)
    lib = CountingLib(_lib.lib())
    monkeypatch.setattr(E, "lib", lambda: lib)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    H, W = 2 * Ho, 2 * Wo
    x = torch.randn(B * T, Cs, H, W, generator=g)
    attn = torch.softmax(torch.randn(nh, B, T, H // ratio, W // ratio, generator=g), dim=2)
    wt = torch.randn(Kc, Cs, 4, 4, generator=g) * 0.1
    gy = torch.randn(B * T, Kc, Ho, Wo, generator=g)
    gskip = torch.randn(B, Cs, H, W, generator=g)
    extra = torch.randn(B * T, Cs, H, W, generator=g)
    valid = torch.ones(B, T, dtype=torch.bool)
    for b, t in pad:
        valid[b, t] = False
    x.view(B, T, Cs, H, W)[~valid] = float("nan")
    attn[:, ~valid] = float("nan")
    vd = valid.view(-1).int().to(dev) if pad else None
    p = {"w": wt.to(dev)}
    ctx = E.Ctx(p, {}, {"w": torch.zeros_like(p["w"])}, E.Workspace(dev), True, E.Tape())
    xd, ad = x.to(dev), attn.to(dev)
    y = E.conv2d(ctx, [xd], "w", None, 4, 2, 1, _lib.PAD_REFLECT if reflect else _lib.PAD_ZEROS, vd)
    if second:
        ed = extra.to(dev)
        ctx.tape.record(lambda: ctx.tape.add_grad(xd, ed, own=False))        # runs between the two backward launches
    out = E.temporal_aggregate(ctx, xd.view(B, T, Cs, H, W), ad, vd, nh)
    ctx.tape.grads[y.data_ptr()] = gy.to(dev)
    ctx.tape.grads[out.data_ptr()] = gskip.to(dev)
    ctx.tape.backward()
    torch.cuda.synchronize()
    assert not ctx.tape.skip_terms
    gx = ctx.tape.grads[xd.data_ptr()].cpu()
    assert bool(torch.isfinite(gx).all()), "non-finite values (a padded frame was read?)"
    if pad and not second:
        assert bool((bits(gx.view(B, T, Cs, H, W)[~valid]) == 0).all()), "gradient of a padded frame is not 0"
    return gx, lib.count


CASES = {
    #                         B  T  Kc  Ho  Wo  Cs   nh ratio
    "base_cpg4":             (2, 3, 24, 8, 32, 64, 16, 8, {}),
    "base_cpg4_no_reflect":  (2, 3, 24, 8, 32, 64, 16, 8, dict(reflect=False)),
    "cpg8":                  (2, 3, 24, 8, 32, 128, 16, 8, {}),
    "cpg16":                 (2, 3, 24, 8, 32, 64, 4, 8, {}),
    "partial_tiles":         (2, 3, 72, 12, 40, 64, 16, 8, {}),
    "ratio2":                (2, 3, 24, 8, 32, 64, 16, 2, {}),
    "ratio1":                (2, 3, 24, 8, 32, 64, 16, 1, {}),
    "cs48_csp64":            (2, 3, 24, 8, 32, 48, 12, 8, {}),
    "one_padded_frame":      (2, 3, 24, 8, 32, 64, 16, 8, dict(pad=((1, 2),))),
}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_skip_term_has_the_bits_of_the_two_step_path(name, monkeypatch):
    *shape, kw = CASES[name]
    two, n2 = run(monkeypatch, False, *shape, **kw)
    one, n1 = run(monkeypatch, True, *shape, **kw)
    assert n2.get("c2s_temporal_aggregate_bwd") == 1 and n2.get("c2s_conv4x4s2_dgrad_winograd") == 1
    assert "c2s_conv4x4s2_dgrad_winograd_skip" not in n2 and "c2s_temporal_aggregate_bwd_skip" not in n2
    assert n1.get("c2s_temporal_aggregate_bwd_skip") == 1 and n1.get("c2s_conv4x4s2_dgrad_winograd_skip") == 1
    assert "c2s_conv4x4s2_dgrad_winograd" not in n1 and "c2s_agg_skip_term" not in n1
    assert bool((bits(one) == bits(two)).all()), f"{int((bits(one) != bits(two)).sum())} elements differ"


def test_two_channels_per_head_take_the_two_step_path(monkeypatch):
    shape = (2, 3, 24, 8, 32, 64, 32, 8)
    two, _ = run(monkeypatch, False, *shape)
    one, n1 = run(monkeypatch, True, *shape)
    assert n1.get("c2s_temporal_aggregate_bwd") == 1 and n1.get("c2s_conv4x4s2_dgrad_winograd") == 1
    assert "c2s_conv4x4s2_dgrad_winograd_skip" not in n1 and "c2s_temporal_aggregate_bwd_skip" not in n1
    assert bool((bits(one) == bits(two)).all())


def test_a_second_consumer_materialises_the_pending_term(monkeypatch):
    shape = (2, 3, 24, 8, 32, 64, 16, 8)
    two, _ = run(monkeypatch, False, *shape, second=True, pad=((0, 1),))
    one, n1 = run(monkeypatch, True, *shape, second=True, pad=((0, 1),))
    assert n1.get("c2s_temporal_aggregate_bwd_skip") == 1 and n1.get("c2s_agg_skip_term") == 1
    assert n1.get("c2s_conv4x4s2_dgrad_winograd") == 1 and "c2s_conv4x4s2_dgrad_winograd_skip" not in n1
    assert bool((bits(one) == bits(two)).all())


def test_train_step_of_a_small_utae_is_bit_identical_with_the_switch_on_and_off(monkeypatch):
    import crop2seg_amd as C2S
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    from crop2seg_amd.backbones.functional import DropoutState
    from crop2seg_amd.learning.utils import TrainStep
    from oracle import seeded
    x, dates, y = seeded.make_inputs(2, 3, 10, 64, 64, 91, [3, 2])          # a padded frame in the second series
    x, dates, y = x.cuda(), dates.cuda(), y.cuda()
    res, counts = {}, {}
    for fused in (False, True):
        torch.manual_seed(0)
        net = C2S.UTAE(input_dim=10, out_conv=[32, 15])
        ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict(seeded.make_state(ks, 3, "tame"))
        net = net.cuda().train()
        monkeypatch.setattr(E, "AGG_SKIP_TERM", fused)
        lib = CountingLib(_lib.lib())
        monkeypatch.setattr(E, "lib", lambda: lib)
        step = TrainStep(net, num_classes=15)
        loss, logits = step(x, dates, y, dropout_state=DropoutState(), apply_update=False)
        torch.cuda.synchronize()
        res[fused] = (loss.clone(), logits.clone(), step.flat_grad.clone())
        counts[fused] = lib.count
    assert counts[True].get("c2s_conv4x4s2_dgrad_winograd_skip", 0) >= 1 and "c2s_agg_skip_term" not in counts[True]
    assert "c2s_conv4x4s2_dgrad_winograd_skip" not in counts[False]
    for a, b, what in zip(res[False], res[True], ("loss", "logits", "flat_grad")):
        assert bool(torch.isfinite(a).all()), what
        assert bool((bits(a) == bits(b)).all()), what
