"""Pin the CPU oracle (oracle/crop2seg_oracle.py) against outputs of the imported reference
(tests/golden/*.npz, written by oracle/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import golden_names
from oracle import crop2seg_oracle as O

# structurally-zero gradients: softmax shift invariance / bias followed by BatchNorm
def _abs_only(name, training):
    if name.endswith("attention_head.fc1_k.bias"):
        return True
    if not training:
        return False
    if name.startswith("up_blocks") and name.endswith(".0.bias"):
        return True
    if name.startswith("out_conv") and name.endswith(".bias") and name.split(".")[-2] in ("0", "3"):
        return True
    return name in ("temporal_encoder.mlp.0.bias", "temporal_encoder.inconv.bias", "temporal_encoder.in_norm.bias")


def _forward(g, dtype):
    """Oracle forward of fixture `g` in `dtype`: logits, attention, loss, boundary logits (or None), BatchNorm updates."""
    bn = O.BNState()
    kw = g.dropout_kwargs()
    if g.cfg.model == "wtae":
        kw.pop("mlp_keep", None)
    sd, x = g.sd, g.x
    if dtype != torch.float32:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        x, kw = x.to(dtype), {k: v.to(dtype) for k, v in kw.items()}
    with torch.no_grad():
        logits, att = O.forward(sd, x, g.dates, g.cfg, training=g.training, bn=bn, **kw)
        loss = O.cross_entropy(logits, g.y, g.cfg.out_conv[-1])
        out_b = None
        if g.cfg.add_boundary_loss:          # second head + focal term (utae.py:236-238; src/learning/utils.py:283-285,318-324)
            from oracle import tail_oracle as TO
            out_b = O.LAST_BOUNDARY[0]
            loss = loss + TO.focal_ce(out_b, TO.boundary_target(g.y, 15), 2.0)
    return logits, att, loss, out_b, bn.updates


class _Anchor:
    """The bounds below were set against the fp32 summation order of the CPU libraries (oneDNN, MKL) the goldens were written
    with; another host's vector ISA or thread count rounds differently, by more than the tightest bounds (measured: attention
    up to 12x its 2e-6 bound, logits up to 3x, with the oracle itself unchanged).  Each check therefore first applies its bound
    to the fp32 oracle; only if that fails does it require the reference's fp32 output to lie within 5 x this host's own fp32
    rounding of the fp64 oracle (measured <= 4.5x over 1 thread, AVX2-only and scalar builds) -- the fp64-anchored protocol of
    the backward test.  A wrong oracle is off by O(1) under either form."""

    FACTOR = 5.0

    def __init__(self, g):
        self.g, self._r64 = g, None

    def r64(self):
        if self._r64 is None:
            self._r64 = _forward(self.g, torch.float64)
        return self._r64

    def close(self, got, ref, bound, got64):
        got, ref = got.double(), ref.double()
        if float((got - ref).abs().max()) <= bound:
            return True
        got64 = got64().double()                 # evaluated only where the host's fp32 rounding differs
        rounding = float((got - got64).abs().max())
        return float((got64 - ref).abs().max()) <= self.FACTOR * rounding

    def same_argmax(self, logits, ref_logits):
        """Class maps equal; failing that, every differing pixel is one where the fp64 oracle's top-2 margin lies within the
        fp32 rounding band (a tie that the summation order decides)."""
        a, b = logits.argmax(1), ref_logits.argmax(1)
        if torch.equal(a, b):
            return True
        l64 = self.r64()[0]
        band = self.FACTOR * float((logits.double() - l64).abs().max())
        top2 = l64.topk(2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1])[a != b]
        return bool((margin <= band).all()) and torch.equal(l64.argmax(1)[a == b], b[a == b])


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_reference_forward(goldens, name):
    g = goldens(name)
    logits, att, loss, out_b, bn_updates = _forward(g, torch.float32)
    A = _Anchor(g)
    if out_b is not None:
        ref_b = torch.from_numpy(g.z["logits_b"])
        assert A.close(out_b, ref_b, 2e-5 * float(ref_b.abs().max()), lambda: A.r64()[3])
    ref_logits = torch.from_numpy(g.z["logits"])
    ref_att = torch.from_numpy(g.z["att"])
    scale = ref_logits.abs().max()
    # train mode under weight_init-style BN gains is ill-conditioned: the fp32 reference differs from
    # ITSELF by 1e-4 between 1 and 8 CPU threads
    tol = 5e-4 if (g.training and g.meta["flavour"] == "wi") else 2e-5
    assert A.close(logits, ref_logits, tol * float(scale), lambda: A.r64()[0]), (logits - ref_logits).abs().max() / scale
    assert A.close(att, ref_att, 2e-6, lambda: A.r64()[1]), (att - ref_att).abs().max()
    ref_loss = torch.tensor(float(g.z["loss"]))
    assert A.close(loss.reshape(()), ref_loss, 1e-5 * abs(float(ref_loss)), lambda: A.r64()[2].reshape(())), (float(loss), float(ref_loss))
    if not g.training:
        # argmax class map bit-exact (ties -> lowest index, like torch.argmax)
        assert A.same_argmax(logits, ref_logits)
    else:
        for k in g.z.files:
            if k.startswith("bn/") and not g.dummy_pass_pollutes(k[3:]):
                ref = torch.from_numpy(g.z[k])
                got = bn_updates[k[3:]]
                assert A.close(got, ref, 1e-5 * max(1.0, float(ref.abs().max())), lambda: A.r64()[4][k[3:]]), k


@pytest.mark.parametrize("name", golden_names())
def test_oracle_matches_reference_backward(goldens, name):
    g = goldens(name)
    kw = g.dropout_kwargs()
    if g.cfg.model == "wtae":
        kw.pop("mlp_keep", None)
    _, loss, grads, _ = O.loss_and_grads(g.sd, g.x, g.dates, g.y, g.cfg, g.training, **kw)
    names = g.grad_names()
    if not names:
        pytest.skip("forward-only fixture (oracle/make_golden.py says why)")
    assert set(names) == set(grads.keys())
    gmax = max(float(g.z[f"grad/{n}/norm"]) for n in names)
    # eval mode: tight against the reference's gradients.  train mode: fp64-anchored criterion (Golden.fp64_anchor).
    for n in names:
        if g.training:
            g.check_train_grad(n, grads[n], gmax, _abs_only(n, True))
            continue
        err, scale, ref_norm, got_norm = g.check_grad(n, grads[n])
        if _abs_only(n, False) or ref_norm < 1e-7 * gmax:
            assert err <= 1e-5 * gmax, (n, err, gmax)
        else:
            assert err <= 2e-4 * scale + 1e-7 * gmax, (n, err / max(scale, 1e-30))


def test_oracle_fp64_runs(goldens):
    """The functional oracle runs in float64 (the reference cannot: temp_shared_block.py:25)."""
    g = goldens("utae_eval_pad_wi")
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in g.sd.items()}
    with torch.no_grad():
        l64, _ = O.forward(sd64, g.x.double(), g.dates, g.cfg)
    ref = torch.from_numpy(g.z["logits"]).double()
    assert l64.dtype == torch.float64
    assert (l64 - ref).abs().max() <= 1e-4 * ref.abs().max()


def test_padded_frames_semantics():
    """A padded frame leaves the encoder as exactly pad_value and gets exactly zero attention
    (SURVEY Appendix N.5)."""
    g = torch.Generator().manual_seed(0)
    cfg = O.BackboneConfig()
    x = torch.randn(1, 3, 10, 16, 16, generator=g)
    x[0, 2] = 0
    from oracle import seeded
    ks = [("in_conv.conv.conv.0.weight", (64, 10, 3, 3)), ("in_conv.conv.conv.0.bias", (64,)),
          ("in_conv.conv.conv.1.weight", (64,)), ("in_conv.conv.conv.1.bias", (64,)),
          ("in_conv.conv.conv.3.weight", (64, 64, 3, 3)), ("in_conv.conv.conv.3.bias", (64,)),
          ("in_conv.conv.conv.4.weight", (64,)), ("in_conv.conv.conv.4.bias", (64,))]
    sd = seeded.make_state(ks, 3, "tame")
    out = O.conv_block(x, sd, "in_conv", 2, "group", cfg, False, None, 0.0)
    assert torch.equal(out[0, 2], torch.zeros_like(out[0, 2]))
    assert out[0, :2].abs().sum() > 0


def test_oracle_adam_matches_torch_optim():
    """O.adam_step is the optimiser the HIP Adam kernel is judged against: pin it to torch.optim.Adam itself
    (defaults of the reference's train.py:454: lr 1e-3, betas (0.9, 0.999), eps 1e-8, no weight decay)."""
    g = torch.Generator().manual_seed(3)
    shapes = {"a": (64, 10, 3, 3), "b": (64,), "c": (1000,)}
    p_ref = {k: torch.nn.Parameter(torch.randn(s, generator=g)) for k, s in shapes.items()}
    p = {k: v.detach().clone() for k, v in p_ref.items()}
    m = {k: torch.zeros(s) for k, s in shapes.items()}
    v = {k: torch.zeros(s) for k, s in shapes.items()}
    opt = torch.optim.Adam(list(p_ref.values()), lr=1e-3)
    for step in range(1, 8):
        grads = {k: torch.randn(s, generator=g) * (10.0 ** (step % 3 - 1)) for k, s in shapes.items()}
        for k in shapes:
            p_ref[k].grad = grads[k].clone()
        opt.step()
        O.adam_step(p, grads, m, v, step)
        for k in shapes:
            assert float((p[k] - p_ref[k].detach()).abs().max()) <= 2e-7 * max(1.0, float(p_ref[k].abs().max())), (k, step)
