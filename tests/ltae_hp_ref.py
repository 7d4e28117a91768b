"""tests/ltae_ref.py for any (n_head, d_k, d_v): the float64 reference of the L-TAE attention block and its per-element
first-order rounding bounds A, with the head count nh, the key width dk and the head width dv = d_model / n_head as arguments
where that module has the constants 16, 4, 16.  Same formulas, same outputs, same A_* arrays line by line
(tests/test_ltae_hparams.py holds the two against each other at 16 / 4 / 16 and this one against torch autograd elsewhere);
the bound constants are ltae_ref.C_KERNEL, unchanged.  CPU only.
"""
import math

import torch

from ltae_ref import C_KERNEL, U, pixel_subset  # noqa: F401  (re-exported: one set of constants for both references)


def state(C, nh, dk, dv, flavour="tame", seed=21):
    """Seeded parameters of the block under the prefix "te", in the reference's shapes (tae.py:355-449)."""
    from oracle import seeded
    dm = nh * dv
    ks = [("te.inconv.weight", (dm, C, 1)), ("te.inconv.bias", (dm,)), ("te.attention_head.Q", (nh, 1, dk)),
          ("te.attention_head.fc1_k.weight", (nh * dk, dm)), ("te.attention_head.fc1_k.bias", (nh * dk,)),
          ("te.in_norm.weight", (C,)), ("te.in_norm.bias", (C,))]
    return seeded.make_state(ks, seed, flavour)


def sinusoid_table(dates, nh, dv, period=1000.0):
    """The default positional table [B,T,nh*dv] (the sinusoid of d = dv repeated over the nh heads, float32 arguments as the
    oracle and the kernel compute them) and its bound: an argument rounded in float32 moves sin / cos by u |arg|."""
    i = torch.arange(dv, dtype=torch.float32)
    denom = torch.pow(torch.tensor(period, dtype=torch.float32), 2 * torch.div(i, 2, rounding_mode="floor") / dv)
    arg = dates.to(torch.float32)[..., None] / denom
    tab = torch.where(i % 2 == 0, torch.sin(arg), torch.cos(arg)).double()
    return tab.repeat(1, 1, nh), (arg.double().abs() + 1.0).repeat(1, 1, nh)


def params_of(sd, nh, dk, dv, prefix="te"):
    """The block's parameters from a state dict, in the shapes ltae_ref takes."""
    C = sd[prefix + ".inconv.weight"].shape[1]
    dm = nh * dv
    return {"gamma": sd[prefix + ".in_norm.weight"], "beta": sd[prefix + ".in_norm.bias"],
            "Wc": sd[prefix + ".inconv.weight"].reshape(dm, C), "bc": sd[prefix + ".inconv.bias"],
            "Q": sd[prefix + ".attention_head.Q"].reshape(nh, dk), "Wk": sd[prefix + ".attention_head.fc1_k.weight"],
            "bk": sd[prefix + ".attention_head.fc1_k.bias"]}


def ltae_hp_ref(x, valid, p, pe, nh, dk, dv, A_pe=None, mask=None, g_emb=None, g_attn=None, pixels=None, eps=1e-5, chunk=2048,
             dtype=torch.float64, norm="two_pass", bounds=True):
    """Reference forward and backward of the block.

    nh heads of width dv (d_model dm = nh * dv), key width dk; the 16 / 4 / 256 below are ltae_ref's, read nh / dk / dm.
    x [B,T,C,HW] (any float); valid [B,T] bool; p: dict gamma, beta [C], Wc [256,C], bc [256], Q [16,4], Wk [64,256],
    bk [64]; pe [B,T,256] positional table, A_pe its bound (None: exact); mask [16,B,T,HW] keep * scale (None: no
    dropout); g_emb [B,256,HW] / g_attn [16,B,T,HW] upstream gradients (either may be None; both None: forward only);
    pixels: flat pixel indices for the pixel-local outputs (None: all).  dtype float32 gives a plain fp32 evaluation of the
    same formulas (its bounds are not computed).  norm="naive": one-pass variance (for the checker's own tests).

    Returns {name: value} and {name: A}: attn_pre / attn [N,16,T], emb [N,256], gx [N,T,C] for the pixel subset (order of
    `pixels`); dgamma, dbeta, gWc, gbc, gQ, gWk, gbk, gpe [B,T,256], gs0 [B,T,16] summed over every pixel."""
    B, T, C, HW = x.shape
    P = B * HW
    dm = nh * dv
    G = nh
    cpg = C // G
    f = lambda t: t.detach().to(dtype).cpu() if t is not None else None      # noqa: E731
    gam, bet, Wc, bc, Q, Wk, bk = (f(p[k]) for k in ("gamma", "beta", "Wc", "bc", "Q", "Wk", "bk"))
    pe = f(pe)
    A_pe = torch.zeros_like(pe) if A_pe is None else f(A_pe).double()
    bwd = g_emb is not None or g_attn is not None
    sel = torch.arange(P) if pixels is None else pixels
    want = torch.zeros(P, dtype=torch.bool)
    want[sel] = True
    pos = torch.full((P,), -1, dtype=torch.int64)
    pos[sel] = torch.arange(sel.numel())
    out, Aout = {}, {}
    N0 = sel.numel()
    for k, shp in (("attn_pre", (N0, nh, T)), ("attn", (N0, nh, T)), ("emb", (N0, dm)), ("gx", (N0, T, C))):
        out[k] = torch.zeros(shp, dtype=dtype)
        Aout[k] = torch.zeros(shp, dtype=torch.float64)
    sums = {"dgamma": (C,), "dbeta": (C,), "gWc": (dm, C), "gbc": (dm,), "gQ": (nh, dk), "gWk": (nh * dk, dm),
            "gbk": (nh * dk,), "gpe": (B, T, dm), "gs0": (B, T, nh)}
    for k, shp in sums.items():
        out[k] = torch.zeros(shp, dtype=torch.float64)
        Aout[k] = torch.zeros(shp, dtype=torch.float64)
    aW = lambda t: t.double().abs()      # noqa: E731
    inv_sdk = 1.0 / math.sqrt(dk)
    # chunks never straddle a batch element: gpe / gs0 are per-b sums
    starts = [(b, s0) for b in range(B) for s0 in range(0, HW, chunk)]
    for b, s0 in starts:
        s1 = min(s0 + chunk, HW)
        flat = torch.arange(b * HW + s0, b * HW + s1)
        if not bwd:                       # forward only: just the pixels asked for
            flat = flat[want[flat]]
            if flat.numel() == 0:
                continue
        s_idx = flat - b * HW
        N = flat.numel()
        xp = x[b][..., s_idx].permute(2, 0, 1).contiguous().to(dtype)                   # [N,T,C]
        vb = valid[b].bool()
        # ---- GroupNorm over (C/16 channels x all T)
        xg = xp.view(N, T, G, cpg)
        if norm == "naive":
            m = xg.mean((1, 3))
            var = ((xg * xg).view(N, T, G, cpg).permute(0, 2, 1, 3).reshape(N, G, -1).cumsum(-1)[..., -1] / (T * cpg)
                   - m * m).clamp_min(0)
        else:
            m = xg.mean((1, 3))
        d = xg - m[:, None, :, None]
        if norm != "naive":
            var = (d * d).mean((1, 3))
        r = 1.0 / torch.sqrt(var + eps)
        xhat = (d * r[:, None, :, None]).view(N, T, C)
        y = xhat * gam + bet
        e = y @ Wc.T + bc + pe[b]                                             # [N,T,256]
        k = e @ Wk.T + bk                                                     # [N,T,64]
        s = torch.einsum("nthd,hd->nht", k.view(N, T, nh, dk), Q) * inv_sdk  # [N,16,T]
        s = s.masked_fill(~vb[None, None], -1e6)
        a_pre = torch.softmax(s, dim=-1)
        mk = torch.ones(N, nh, T, dtype=dtype) if mask is None else mask[:, b][..., s_idx].permute(2, 0, 1).to(dtype)
        a = a_pre * mk
        e4 = e.view(N, T, nh, dv)
        emb = torch.einsum("nht,nthj->nhj", a, e4).reshape(N, dm)
        if bounds:
            X = xp.double().abs()
            md, dd, rd = m.double(), d.double(), r.double()
            xh, yd, ed, kd = xhat.double(), y.double(), e.double(), k.double()
            # mean: sum rounding; variance: the rounding of (x - m) -- |x| + |m| -- squared against |x - m|, + the sum
            A_m = X.view(N, T, G, cpg).mean((1, 3))
            A_var = var.double() + 2 * (dd.abs() * (X.view(N, T, G, cpg) + md.abs()[:, None, :, None])).mean((1, 3))
            A_r = rd * A_var / (2 * (var.double() + eps)) + rd
            A_xh = (rd[:, None, :, None] * (A_m[:, None, :, None] + X.view(N, T, G, cpg) + md.abs()[:, None, :, None])
                    + dd.abs() * A_r[:, None, :, None]).view(N, T, C)
            A_y = aW(gam) * (A_xh + xh.abs()) + aW(bet)
            A_e = (A_y + yd.abs()) @ aW(Wc).T + aW(bc) + pe[b].double().abs() + A_pe[b]
            A_k = (A_e + ed.abs()) @ aW(Wk).T + aW(bk)
            A_s = torch.einsum("nthd,hd->nht", (A_k + kd.abs()).view(N, T, nh, dk), aW(Q)) * inv_sdk
            sd_ = s.double()
            As_hat = (A_s + (sd_ - sd_.max(-1, keepdim=True).values).abs() + 1.0) * vb[None, None]
            ap = a_pre.double()
            A_ap = ap * (As_hat + (ap * As_hat).sum(-1, keepdim=True)) + ap
            mkd = mk.double()
            A_a = A_ap * mkd
            ad = a.double()
            A_emb = torch.einsum("nht,nthj->nhj", A_a + ad, ed.abs().view(N, T, nh, dv)) + \
                torch.einsum("nht,nthj->nhj", ad, A_e.view(N, T, nh, dv))
            A_emb = A_emb.reshape(N, dm)
        w = want[flat]
        if bool(w.any()):
            o = pos[flat[w]]
            out["attn_pre"][o], out["attn"][o], out["emb"][o] = a_pre[w], a[w], emb[w]
            if bounds:
                Aout["attn_pre"][o], Aout["attn"][o], Aout["emb"][o] = A_ap[w], A_a[w], A_emb[w]
        if not bwd:
            continue
        # ---- backward
        ge = torch.zeros(N, dm, dtype=dtype) if g_emb is None else g_emb[b][:, s_idx].T.to(dtype)     # [N,256]
        gA = torch.zeros(N, nh, T, dtype=dtype) if g_attn is None else g_attn[:, b][..., s_idx].permute(2, 0, 1).to(dtype)
        ge4 = ge.view(N, nh, dv)
        ga = gA + torch.einsum("nhj,nthj->nht", ge4, e4)                     # d a  (values path of emb + direct)
        gap = ga * mk                                                         # d a_pre
        dot = (a_pre * gap).sum(-1, keepdim=True)
        gs = a_pre * (gap - dot)                                              # softmax backward (0 on padded frames)
        gk = (gs.permute(0, 2, 1)[..., None] * Q * inv_sdk).reshape(N, T, nh * dk)
        gE = torch.einsum("nht,nhj->nthj", a, ge4).reshape(N, T, dm) + gk @ Wk   # d e
        gy = gE @ Wc                                                          # [N,T,C]
        gxh = (gy * gam).view(N, T, G, cpg)
        xh4 = xhat.view(N, T, G, cpg)
        m1 = gxh.mean((1, 3), keepdim=True)
        m2 = (gxh * xh4).mean((1, 3), keepdim=True)
        gx = (r[:, None, :, None] * (gxh - m1 - xh4 * m2)).view(N, T, C)
        out["dgamma"] += (gy * xhat).double().sum((0, 1))
        out["dbeta"] += gy.double().sum((0, 1))
        out["gWc"] += torch.einsum("ntd,ntc->dc", gE.double(), y.double())
        out["gbc"] += gE.double().sum((0, 1))
        out["gQ"] += torch.einsum("nht,nthd->hd", gs.double(), k.double().view(N, T, nh, dk)) * inv_sdk
        out["gWk"] += torch.einsum("ntk,ntd->kd", gk.double(), e.double())
        out["gbk"] += gk.double().sum((0, 1))
        out["gpe"][b] += gE.double().sum(0)
        out["gs0"][b] += gs.double().sum(0).T
        if bounds:
            gad, gapd, gsd, gkd, gEd, gyd = ga.double(), gap.double(), gs.double(), gk.double(), gE.double(), gy.double()
            A_ga = gA.double().abs() + torch.einsum("nhj,nthj->nht", ge.double().abs().view(N, nh, dv),
                                                     (ed.abs() + A_e).view(N, T, nh, dv))
            A_gap = A_ga * mkd
            A_dot = (A_ap * gapd.abs() + ap * (A_gap + gapd.abs())).sum(-1, keepdim=True)
            A_gs = A_ap * (gapd - dot.double()).abs() + ap * (A_gap + A_dot + gapd.abs() + dot.double().abs())
            A_gk = ((A_gs + gsd.abs()).permute(0, 2, 1)[..., None] * aW(Q) * inv_sdk).reshape(N, T, nh * dk)
            A_gE = (torch.einsum("nht,nhj->nthj", A_a + ad, ge.double().abs().view(N, nh, dv)).reshape(N, T, dm)
                    + (A_gk + gkd.abs()) @ aW(Wk))
            A_gy = (A_gE + gEd.abs()) @ aW(Wc)
            gxhd = gxh.double()
            A_gxh = (aW(gam) * (A_gy + gyd.abs())).view(N, T, G, cpg)
            xh4d, A_xh4 = xh.view(N, T, G, cpg), A_xh.view(N, T, G, cpg)
            A_m1 = A_gxh.mean((1, 3), keepdim=True)
            A_m2 = (A_gxh * xh4d.abs() + gxhd.abs() * A_xh4 + (gxhd * xh4d).abs()).mean((1, 3), keepdim=True)
            m1d, m2d = m1.double(), m2.double()
            inner = gxhd - m1d - xh4d * m2d
            A_gx = (A_r[:, None, :, None] * inner.abs()
                    + rd[:, None, :, None] * (A_gxh + A_m1 + xh4d.abs() * A_m2 + A_xh4 * m2d.abs()
                                              + gxhd.abs() + m1d.abs() + (xh4d * m2d).abs())).view(N, T, C)
            Aout["dgamma"] += (A_gy * xh.abs() + gyd.abs() * A_xh + (gyd * xh).abs()).sum((0, 1))
            Aout["dbeta"] += (A_gy + gyd.abs()).sum((0, 1))
            Aout["gWc"] += torch.einsum("ntd,ntc->dc", A_gE + gEd.abs(), yd.abs()) + torch.einsum("ntd,ntc->dc", gEd.abs(), A_y)
            Aout["gbc"] += (A_gE + gEd.abs()).sum((0, 1))
            Aout["gQ"] += (torch.einsum("nht,nthd->hd", A_gs + gsd.abs(), kd.abs().view(N, T, nh, dk))
                           + torch.einsum("nht,nthd->hd", gsd.abs(), A_k.view(N, T, nh, dk))) * inv_sdk
            Aout["gWk"] += torch.einsum("ntk,ntd->kd", A_gk + gkd.abs(), ed.abs()) + torch.einsum("ntk,ntd->kd", gkd.abs(), A_e)
            Aout["gbk"] += (A_gk + gkd.abs()).sum((0, 1))
            Aout["gpe"][b] += (A_gE + gEd.abs()).sum(0)
            Aout["gs0"][b] += (A_gs + gsd.abs()).sum(0).T
        if bool(w.any()):
            o = pos[flat[w]]
            out["gx"][o] = gx[w]
            if bounds:
                Aout["gx"][o] = A_gx[w]
    return out, Aout
