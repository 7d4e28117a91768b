"""CPU checks of tests/ltae_ref.py: the float64 reference agrees with the pinned oracle (forward) and with float64 autograd
(the explicit backward), a plain float32 evaluation of the block meets the bound with room to spare, and the bound rejects
the local errors a kernel could make: a time step missing from one softmax denominator, a keep flag taken from the other
half of its hash pair, weight on a padded frame, a one-pass variance, a gradient row from the neighbouring pixel, one
tile's partial missing from a parameter sum, the positional entry of t+1 used for t."""
import math

import pytest
import torch

import conv_ref
import ltae_ref as R
from oracle import crop2seg_oracle as O
from oracle import seeded

C_CPU = R.C_KERNEL       # the kernels' constants: a float32 evaluation stays below half of each
PE_MODES = ("doy", "abs_rel", "linear", "abs_rel_doy", "abs_rel_linear")


def state(C, pe_mode="rel", flavour="tame"):
    ks = [("te.inconv.weight", (256, C, 1)), ("te.inconv.bias", (256,)), ("te.attention_head.Q", (16, 1, 4)),
          ("te.attention_head.fc1_k.weight", (64, 256)), ("te.attention_head.fc1_k.bias", (64,)),
          ("te.in_norm.weight", (C,)), ("te.in_norm.bias", (C,))]
    if pe_mode in ("doy", "abs_rel_doy"):
        ks += [("te.positional_encoder.fc.weight", (16, 365)), ("te.positional_encoder.fc.bias", (16,))]
    if pe_mode in ("linear", "abs_rel_linear"):
        ks += [("te.positional_encoder.fc.weight", (256, 256)), ("te.positional_encoder.fc.bias", (256,))]
    if pe_mode.startswith("abs_rel"):
        ks += [("te.positional_encoder_abs.fc.weight", (16, 365)), ("te.positional_encoder_abs.fc.bias", (16,))]
    return seeded.make_state(ks, 21, flavour)


def case(B, T, C, h, seed=5, pad=True, offset=False, pe_mode="rel", p=0.1):
    """x [B,T,C,h,w] with random finite values on padded frames (trailing runs; batch element 1 keeps one frame)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, C, h, h, generator=g)
    if offset:
        x = x + 20.0
    valid = torch.ones(B, T, dtype=torch.bool)
    if pad and T > 2:
        valid[0, T - 2:] = False
        if B > 1:
            valid[1, 1:] = False
    rel = (5 * torch.arange(T)[None] + torch.arange(B)[:, None]).long()
    dates = torch.stack([rel, (rel * 7 + 11) % 365], -1) if pe_mode.startswith("abs_rel") else (
        (rel * 3 + 2) % 365 if pe_mode == "doy" else rel)
    keep = (torch.rand(16, B * h * h, T, generator=g) >= p).double()
    g_emb = torch.randn(B, 256, h * h, generator=g, dtype=torch.float64)
    g_attn = torch.randn(16, B, T, h * h, generator=g, dtype=torch.float64)
    return x, valid, dates, keep, g_emb, g_attn


def mask_of(keep, B, T, HW, p):
    return keep.view(16, B, HW, T).permute(0, 1, 3, 2) / (1.0 - p)


def cfg_of(pe_mode, p):
    cfg = O.BackboneConfig()
    cfg.pe_mode = pe_mode
    cfg.attn_dropout = p
    return cfg


def table(pe_mode, dates, sd):
    if pe_mode == "rel":
        return R.sinusoid_table(dates)
    names = {"enc.weight": "te.positional_encoder.fc.weight", "enc.bias": "te.positional_encoder.fc.bias",
             "enc2.weight": "te.positional_encoder_abs.fc.weight", "enc2.bias": "te.positional_encoder_abs.fc.bias"}
    return R.pe_table(pe_mode, dates, {k: sd[v] for k, v in names.items() if v in sd})


@pytest.mark.parametrize("pe_mode", ("rel",) + PE_MODES)
def test_forward_agrees_with_the_oracle_in_float64(pe_mode):
    B, T, C, h, p = 2, 7, 64, 3, 0.1
    x, valid, dates, keep, _, _ = case(B, T, C, h, pe_mode=pe_mode)
    sd = {k: v.double() for k, v in state(C, pe_mode).items()}
    emb, attn = O.ltae_attention(x.double(), dates, ~valid, sd, "te", cfg_of(pe_mode, p), keep)
    pe = O.positional_encoding(dates, sd, "te", cfg_of(pe_mode, p), torch.float64)
    tab, A_tab = table(pe_mode, dates, sd)                 # the table the GPU rows use, within its own bound
    assert bool(((tab - pe).abs() <= 4 * R.U * A_tab + 1e-30).all())
    out, _ = R.ltae_ref(x.view(B, T, C, h * h), valid, R.params_of(sd), pe, mask=mask_of(keep, B, T, h * h, p))
    ref_attn = attn.view(16, B, h * h, T).permute(1, 2, 0, 3).reshape(-1, 16, T)
    assert float((out["attn"] - ref_attn).abs().max()) <= 1e-12 * float(ref_attn.abs().max())
    assert float((out["emb"] - emb).abs().max()) <= 1e-12 * float(emb.abs().max())


@pytest.mark.parametrize("pe_mode", ("rel",) + PE_MODES)
def test_explicit_backward_agrees_with_float64_autograd(pe_mode):
    B, T, C, h, p = 2, 9, 128, 3, 0.3
    x, valid, dates, keep, g_emb, g_attn = case(B, T, C, h, seed=8, pe_mode=pe_mode, p=p)
    HW = h * h
    sd = {k: v.double().requires_grad_(True) for k, v in state(C, pe_mode).items()}
    xg = x.double().requires_grad_(True)
    emb, attn = O.ltae_attention(xg, dates, ~valid, sd, "te", cfg_of(pe_mode, p), keep)
    ge = g_emb.view(B, 256, HW).permute(0, 2, 1).reshape(-1, 256)
    ga = g_attn.permute(0, 1, 3, 2).reshape(16, -1, T)
    ((emb * ge).sum() + (attn * ga).sum()).backward()
    pe = O.positional_encoding(dates, sd, "te", cfg_of(pe_mode, p), torch.float64)
    out, _ = R.ltae_ref(x.view(B, T, C, HW), valid, R.params_of(sd), pe.detach(), mask=mask_of(keep, B, T, HW, p),
                        g_emb=g_emb, g_attn=g_attn)

    def close(got, ref, what):
        assert float((got - ref).abs().max()) <= 1e-10 * max(float(ref.abs().max()), 1.0), what   # gbk is 0 up to rounding

    close(out["gx"], xg.grad.view(B, T, C, HW).permute(0, 3, 1, 2).reshape(-1, T, C), "gx")
    close(out["dgamma"], sd["te.in_norm.weight"].grad, "dgamma")
    close(out["dbeta"], sd["te.in_norm.bias"].grad, "dbeta")
    close(out["gWc"], sd["te.inconv.weight"].grad.view(256, C), "gWc")
    close(out["gbc"], sd["te.inconv.bias"].grad, "gbc")
    close(out["gQ"], sd["te.attention_head.Q"].grad.view(16, 4), "gQ")
    close(out["gWk"], sd["te.attention_head.fc1_k.weight"].grad, "gWk")
    close(out["gbk"], sd["te.attention_head.fc1_k.bias"].grad, "gbk")
    if pe_mode != "rel":
        gp, _ = R.pe_param_grads(pe_mode, dates, out["gpe"], torch.zeros_like(out["gpe"]), {})
        for k, v in gp.items():
            name = {"enc": "te.positional_encoder.fc", "enc2": "te.positional_encoder_abs.fc"}[k.split(".")[0]]
            close(v, sd[name + "." + k.split(".")[1]].grad, k)


def _fp32_and_ref(B, T, C, h, offset=False, norm="two_pass", seed=5, pe_shift=None, mask_mut=None):
    p = 0.3
    x, valid, dates, keep, g_emb, g_attn = case(B, T, C, h, seed=seed, offset=offset, p=p)
    HW = h * h
    xs = x.view(B, T, C, HW)
    sd = state(C)
    prm = R.params_of(sd)
    pe, A_pe = R.sinusoid_table(dates)
    mask = mask_of(keep, B, T, HW, p)
    pix = R.pixel_subset(B, HW, n_random=16, edge=20)
    ref, A = R.ltae_ref(xs, valid, prm, pe, A_pe, mask, g_emb, g_attn, pixels=pix)
    pe32 = pe.clone()
    if pe_shift is not None:
        pe32[:, pe_shift] = pe[:, pe_shift + 1]
    m32 = mask if mask_mut is None else mask_mut(mask)
    got, _ = R.ltae_ref(xs, valid, prm, pe32, None, m32, g_emb, g_attn, pixels=pix, dtype=torch.float32, norm=norm,
                        bounds=False)
    return got, ref, A, (xs, valid, prm, pe, m32, g_emb, g_attn)


def ratios(got, ref, A, keys=("attn", "emb", "gx", "dgamma", "dbeta", "gWc", "gbc", "gQ", "gWk", "gbk")):
    # gbk is zero up to rounding (softmax is shift-invariant): no Frobenius bar there, the per-element bound still holds
    return {k: conv_ref.assert_within(k, got[k], ref[k], A[k], C_CPU[k], math.inf if k == "gbk" else 1e-4) for k in keys}


@pytest.mark.parametrize("offset", [False, True])
def test_float32_evaluation_meets_the_bound(offset):
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6, offset=offset)
    r = ratios(got, ref, A)
    assert all(r[k] < C_CPU[k] / 2 for k in r), r


def _rejects(got, ref, A, keys):
    with pytest.raises(AssertionError, match="beyond c|Frobenius"):
        ratios(got, ref, A, keys=keys)


def test_rejects_a_step_missing_from_one_softmax_denominator():
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6)
    n, h, tl = 5, 3, 36                       # last T chunk of a series with every frame valid (batch element 0: 37 valid)
    ap = got["attn_pre"][n, h].clone()
    row = ap / (1 - ap[tl])
    row[tl] = ap[tl]
    got["attn"][n, h] = row * (got["attn"][n, h] / ap.clamp_min(1e-30))
    _rejects(got, ref, A, ("attn",))


def test_rejects_a_keep_flag_from_the_other_half_of_its_hash_pair():
    def mut(mask):
        m = mask.clone()
        diff = (m[:, 0, 0::2][:, :18] != m[:, 0, 1::2][:, :18]).nonzero()
        h, u, s = (int(v) for v in diff[0])
        m[h, 0, 2 * u + 1, s] = m[h, 0, 2 * u, s]
        return m
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6, mask_mut=mut)
    _rejects(got, ref, A, ("attn",))


def test_rejects_weight_on_a_padded_frame():
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6)
    got["attn"][0, 2, 38] = 1e-6                   # pixel 0 of batch element 0: frames 37, 38 padded
    _rejects(got, ref, A, ("attn",))


def test_rejects_one_pass_variance_on_the_offset_case():
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6, offset=True, norm="naive")
    _rejects(got, ref, A, ("attn", "emb", "gx"))


def test_rejects_a_gradient_row_of_the_neighbouring_pixel():
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6)
    got["gx"][4, 10] = got["gx"][5, 10]
    _rejects(got, ref, A, ("gx",))


@pytest.mark.parametrize("key", ["dgamma", "dbeta", "gQ"])
def test_rejects_one_tile_missing_from_a_parameter_sum(key):
    got, ref, A, (xs, valid, prm, pe, m32, g_emb, g_attn) = _fp32_and_ref(2, 39, 64, 8)
    tile, _ = R.ltae_ref(xs[..., 16:32], valid, prm, pe, None, m32[..., 16:32], g_emb[..., 16:32], g_attn[..., 16:32],
                         pixels=torch.arange(0), dtype=torch.float32, bounds=False)
    got[key] = got[key] - tile[key]
    _rejects(got, ref, A, (key,))


def test_rejects_the_positional_entry_of_the_next_step():
    got, ref, A, _ = _fp32_and_ref(2, 39, 64, 6, pe_shift=3)
    _rejects(got, ref, A, ("attn", "emb"))
