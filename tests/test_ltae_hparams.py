"""CPU side of the L-TAE hyper-parameters n_head, d_model, d_k away from 16 / 256 / 4:

* tests/ltae_hp_ref.py, the float64 reference with (n_head, d_k, d_v) as arguments, equals tests/ltae_ref.py at 16 / 4 / 16
  (values and the rounding-propagation arrays A alike), equals float64 autograd of the pinned oracle at four other
  triples, and a wrong 1/sqrt(d_k) planted in a float32 evaluation is caught by the bound;
* the constructors: the model classes open d_model (128, 256, 512 at n_head = 16, d_k = 4) and build the reference's
  state_dict (keys and shapes of the golden fixture); n_head and d_k away from 16 / 4 stay refused there, as
  tests/test_abi.py holds them -- the kernels, the C ABI and engine.ltae_attention take them
  (tests/test_ltae_hparams_gpu.py); everything refused raises in the constructor, naming the offending value;
* the fixture of tools/make_golden_ltae_hparams.py exists and loads.
"""
import json
import os

import numpy as np
import pytest
import torch

import ltae_hp_ref as H
import ltae_ref as R
from oracle import crop2seg_oracle as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["timeunet_eval_h16m512k4_tame"]
# (n_head, d_k, d_v) of the autograd cases: head widths 32, 16, 8 and a d_k that is no power of two
TRIPLES = [(8, 8, 32), (8, 2, 16), (16, 1, 8), (16, 6, 16)]
KEYS = ("attn", "emb", "gx", "dgamma", "dbeta", "gWc", "gbc", "gQ", "gWk", "gbk")


state = H.state


def case(B, T, C, h, nh, dv, seed=5, p=0.1):
    """As tests/test_ltae_reference.case: random finite values on padded frames (trailing runs; element 1 keeps one)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, h, h, generator=g)
    valid = torch.ones(B, T, dtype=torch.bool)
    if T > 2:
        valid[0, T - 2:] = False
        if B > 1:
            valid[1, 1:] = False
    dates = (5 * torch.arange(T)[None] + torch.arange(B)[:, None]).long()
    keep = (torch.rand(nh, B * h * h, T, generator=g) >= p).double()
    g_emb = torch.randn(B, nh * dv, h * h, generator=g, dtype=torch.float64)
    g_attn = torch.randn(nh, B, T, h * h, generator=g, dtype=torch.float64)
    return x, valid, dates, keep, g_emb, g_attn


def mask_of(keep, nh, B, T, HW, p):
    return keep.view(nh, B, HW, T).permute(0, 1, 3, 2) / (1.0 - p)


def cfg_of(nh, dk, dv, p):
    cfg = O.BackboneConfig(n_head=nh, d_model=nh * dv, d_k=dk)
    cfg.attn_dropout = p
    return cfg


def test_equals_ltae_ref_at_the_default_hyper_parameters():
    B, T, C, h, p = 2, 7, 64, 3, 0.3
    x, valid, dates, keep, g_emb, g_attn = case(B, T, C, h, 16, 16, p=p)
    HW = h * h
    sd = state(C, 16, 4, 16)
    pe0, A0 = R.sinusoid_table(dates)
    pe1, A1 = H.sinusoid_table(dates, 16, 16)
    assert torch.equal(pe0, pe1) and torch.equal(A0, A1)
    prm0, prm1 = R.params_of(sd), H.params_of(sd, 16, 4, 16)
    assert all(torch.equal(prm0[k], prm1[k]) for k in prm0)
    mask = mask_of(keep, 16, B, T, HW, p)
    pix = R.pixel_subset(B, HW, n_random=4, edge=5)
    ref, A = R.ltae_ref(x.view(B, T, C, HW), valid, prm0, pe0, A0, mask, g_emb, g_attn, pixels=pix)
    got, Ag = H.ltae_hp_ref(x.view(B, T, C, HW), valid, prm1, pe1, 16, 4, 16, A1, mask, g_emb, g_attn, pixels=pix)
    assert set(ref) == set(got) and set(A) == set(Ag)
    for k in ref:       # the same float64 operations in the same order: equal to float64 rounding
        assert float((got[k] - ref[k]).abs().max()) <= 1e-15 * max(float(ref[k].abs().max()), 1.0), k
        assert float((Ag[k] - A[k]).abs().max()) <= 1e-15 * max(float(A[k].abs().max()), 1.0), "A_" + k


@pytest.mark.parametrize("nh,dk,dv", TRIPLES)
def test_equals_float64_autograd(nh, dk, dv):
    B, T, C, h, p = 2, 6, 64, 3, 0.3
    dm = nh * dv
    x, valid, dates, keep, g_emb, g_attn = case(B, T, C, h, nh, dv, seed=8, p=p)
    HW = h * h
    sd = {k: v.double().requires_grad_(True) for k, v in state(C, nh, dk, dv).items()}
    xg = x.double().requires_grad_(True)
    cfg = cfg_of(nh, dk, dv, p)
    emb, attn = O.ltae_attention(xg, dates, ~valid, sd, "te", cfg, keep)
    ge = g_emb.view(B, dm, HW).permute(0, 2, 1).reshape(-1, dm)
    ga = g_attn.permute(0, 1, 3, 2).reshape(nh, -1, T)
    ((emb * ge).sum() + (attn * ga).sum()).backward()
    pe = O.positional_encoding(dates, sd, "te", cfg, torch.float64)
    tab, A_tab = H.sinusoid_table(dates, nh, dv)            # the table the GPU rows use, within its own bound
    assert tab.shape == pe.shape and bool(((tab - pe).abs() <= 4 * R.U * A_tab + 1e-30).all())
    out, _ = H.ltae_hp_ref(x.view(B, T, C, HW), valid, H.params_of(sd, nh, dk, dv), pe.detach(), nh, dk, dv,
                           mask=mask_of(keep, nh, B, T, HW, p), g_emb=g_emb, g_attn=g_attn)

    def close(got, ref, what):
        assert float((got - ref).abs().max()) <= 1e-10 * max(float(ref.abs().max()), 1.0), what

    close(out["attn"], attn.detach().view(nh, B, HW, T).permute(1, 2, 0, 3).reshape(-1, nh, T), "attn")
    close(out["emb"], emb.detach(), "emb")
    close(out["gx"], xg.grad.view(B, T, C, HW).permute(0, 3, 1, 2).reshape(-1, T, C), "gx")
    close(out["dgamma"], sd["te.in_norm.weight"].grad, "dgamma")
    close(out["dbeta"], sd["te.in_norm.bias"].grad, "dbeta")
    close(out["gWc"], sd["te.inconv.weight"].grad.view(dm, C), "gWc")
    close(out["gbc"], sd["te.inconv.bias"].grad, "gbc")
    close(out["gQ"], sd["te.attention_head.Q"].grad.view(nh, dk), "gQ")
    close(out["gWk"], sd["te.attention_head.fc1_k.weight"].grad, "gWk")
    close(out["gbk"], sd["te.attention_head.fc1_k.bias"].grad, "gbk")


def _worst(got, ref, A):
    return {k: float(((got[k].double() - ref[k]).abs() / (R.U * A[k] + 1e-30)).max()) for k in KEYS}


def test_a_wrong_key_scale_is_caught():
    """A float32 evaluation of the block with d_k = 8 meets the kernels' bound; the same evaluation scaling the scores by
    1/2 -- the 1/sqrt(4) of the default d_k -- instead of 1/sqrt(8) does not."""
    nh, dk, dv = 8, 8, 32
    B, T, C, h, p = 2, 7, 64, 3, 0.3
    x, valid, dates, keep, g_emb, g_attn = case(B, T, C, h, nh, dv, p=p)
    HW = h * h
    xs = x.view(B, T, C, HW)
    prm = H.params_of(state(C, nh, dk, dv), nh, dk, dv)
    pe, A_pe = H.sinusoid_table(dates, nh, dv)
    mask = mask_of(keep, nh, B, T, HW, p)
    pix = R.pixel_subset(B, HW, n_random=4, edge=5)
    ref, A = H.ltae_hp_ref(xs, valid, prm, pe, nh, dk, dv, A_pe, mask, g_emb, g_attn, pixels=pix)
    good, _ = H.ltae_hp_ref(xs, valid, prm, pe, nh, dk, dv, None, mask, g_emb, g_attn, pixels=pix, dtype=torch.float32,
                            bounds=False)
    w = _worst(good, ref, A)
    assert all(w[k] <= R.C_KERNEL[k] for k in KEYS), w
    # scores scaled by 1/sqrt(4): Q' = Q sqrt(8)/sqrt(4) under the right scale gives exactly those scores
    bad_prm = dict(prm, Q=prm["Q"] * (8.0 / 4.0) ** 0.5)
    bad, _ = H.ltae_hp_ref(xs, valid, bad_prm, pe, nh, dk, dv, None, mask, g_emb, g_attn, pixels=pix, dtype=torch.float32,
                           bounds=False)
    w = _worst(bad, ref, A)
    assert w["attn"] > R.C_KERNEL["attn"] and w["emb"] > R.C_KERNEL["emb"] and w["gx"] > R.C_KERNEL["gx"], w


# ------------------------------------------------------------------------------------------------ constructors
def _cls(model):
    import crop2seg_amd as C2S
    return {"utae": C2S.UTAE, "timeunet": C2S.TimeUNet_v1, "wtae": C2S.WTAE}[model]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_exists_and_state_dict_matches_reference(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    ctor = meta["ctor"]
    assert set(ctor) == {"n_head", "d_model", "d_k"} and (ctor["n_head"], ctor["d_model"], ctor["d_k"]) == (16, 512, 4)
    for k in ("x", "dates", "y", "wsum", "keys", "shapes"):
        assert k in z.files
    net = _cls(meta["model"])(input_dim=10, out_conv=[32, 15], **ctor)
    assert (net.spec.n_head, net.spec.d_model, net.spec.d_k) == (ctor["n_head"], ctor["d_model"], ctor["d_k"])
    got = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    ref = [(str(k), json.loads(str(s))) for k, s in zip(z["keys"], z["shapes"])]
    assert got == ref
    sd = dict(got)
    nh, dm, dk = ctor["n_head"], ctor["d_model"], ctor["d_k"]
    c_ltae = 64 if meta["model"] == "timeunet" else 128
    assert sd["temporal_encoder.attention_head.Q"] == [nh, 1, dk]
    assert sd["temporal_encoder.attention_head.fc1_k.weight"] == [nh * dk, dm]
    assert sd["temporal_encoder.inconv.weight"] == [dm, c_ltae, 1]
    if meta["model"] == "timeunet":
        assert sd["temporal_encoder.mlp.0.weight"] == [c_ltae, dm]
    assert not any("positional_encoder" in k for k in sd)


@pytest.mark.parametrize("model", ["timeunet", "wtae"])
@pytest.mark.parametrize("d_model", [128, 256, 512])
def test_constructor_accepts(model, d_model):
    net = _cls(model)(input_dim=10, d_model=d_model)
    assert (net.spec.n_head, net.spec.d_model, net.spec.d_k) == (16, d_model, 4)
    sd = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    c_ltae = 64 if model == "timeunet" else 128
    assert sd["temporal_encoder.attention_head.Q"] == (16, 1, 4)
    assert sd["temporal_encoder.attention_head.fc1_k.weight"] == (64, d_model)
    assert sd["temporal_encoder.inconv.weight"] == (d_model, c_ltae, 1)


def test_utae_keeps_d_model_256_like_the_reference():
    with pytest.raises(AssertionError):          # utae.py:179 builds LTAE(mlp=[256,128]); tae.py:404 asserts mlp[0] == d_model
        _cls("utae")(input_dim=10, d_model=128)


@pytest.mark.parametrize("model,kw,names", [
    ("utae", dict(n_head=4), "n_head=4"),
    ("timeunet", dict(n_head=32), "n_head=32"),
    ("timeunet", dict(n_head=16, d_model=1024), "d_model=1024"),
    ("wtae", dict(d_k=33), "d_k=33"),
    ("wtae", dict(d_k=0), "d_k=0"),
    ("utae", dict(n_head=8), "n_head=8"),
    ("timeunet", dict(d_k=8), "d_k=8"),
    ("wtae", dict(d_model=64), "d_model=64"),
    ("utae", dict(n_head=8, use_doy=True), "n_head=8"),
    ("timeunet", dict(n_head=16, d_model=128, use_abs_rel_enc=True), "d_model=128"),
    ("wtae", dict(n_head=8, add_linear=True), "n_head=8"),
    # a width the temporal aggregation's width / n_head in {1, 2, 4, 8, 16} rule rejects (192 / 16 = 12), away from d_model 256
    ("timeunet", dict(d_model=128, encoder_widths=[192, 64, 64, 128], decoder_widths=[32, 32, 64, 128]), "[192]"),
])
def test_constructor_refuses(model, kw, names):
    with pytest.raises(NotImplementedError) as ei:
        _cls(model)(input_dim=10, **kw)
    assert names in str(ei.value), str(ei.value)


def test_long_series_need_the_default_heads():
    """T > 64 with another (n_head, d_model) is refused by _check_inputs before anything touches the device."""
    from crop2seg_amd.backbones import modules as M
    net = _cls("timeunet")(input_dim=10, d_model=128)

    class FakeCuda(torch.Tensor):
        is_cuda = True

    x = torch.zeros(1, 65, 10, 16, 16).as_subclass(FakeCuda)
    with pytest.raises(NotImplementedError, match="d_model=128"):
        M._Backbone._check_inputs(net, x, torch.zeros(1, 65, dtype=torch.long))
