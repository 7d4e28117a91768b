"""Child process of tests/test_ltae_hparams_gpu.py: L-TAE rows at (n_head, d_model, d_k) away from 16 / 256 / 4 against the
float64 reference of tests/ltae_hp_ref.py, in the manner of tests/ltae_ref_worker.py.

argv[1]: JSON list of rows, argv[2]: the bound constants.  Each row prints one line "ROW <json>" (families reached, worst ratio
per output); the process prints LTAE_HP_OK <n> when every row passed.  Optional argv[3]: MiB of the guard-band arena, as in
tests/ltae_ref_worker.py."""
import ctypes
import json
import math
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import conv_ref  # noqa: E402
import ltae_hp_ref as H  # noqa: E402
import ltae_ref as R  # noqa: E402
from ltae_ref_worker import ENC, FROB, run_row_in_arena, thr_scale  # noqa: E402

FOLD = ["te.attention_head.Q", "te.attention_head.fc1_k.weight", "te.attention_head.fc1_k.bias", "te.inconv.weight",
        "te.inconv.bias"]


def dims(row):
    nh, dm, dk = row["nh"], row["dm"], row["dk"]
    return nh, dm, dk, dm // nh


def inputs(row):
    nh, dm, dk, dv = dims(row)
    B, T, C, h, w = row["B"], row["T"], row["C"], row["h"], row["w"]
    g = torch.Generator().manual_seed(row.get("seed", 3))
    sd = H.state(C, nh, dk, dv)
    pe_mode = row.get("pe", "rel")
    if pe_mode != "rel":                        # the learnable encoders' parameters, as tests/test_ltae_reference.state
        import test_ltae_reference as TR
        sd.update({k: v for k, v in TR.state(C, pe_mode).items() if ".positional_encoder" in k})
    x = torch.randn(B, T, C, h, w, generator=g)
    valid = torch.ones(B, T, dtype=torch.bool)
    if row.get("pad") and T > 1:
        valid[0, max(T - 3, 1):] = False        # trailing run; padded frames keep their random finite values
        if B > 1:
            valid[B - 1, 1:] = False            # a batch element with one valid frame
    dates = (5 * torch.arange(T)[None] + torch.arange(B)[:, None]).long()
    if pe_mode.startswith("abs_rel"):
        dates = torch.stack([dates, (dates * 7 + 11) % 365], -1)
    elif pe_mode == "doy":
        dates = (dates * 3 + 2) % 365
    return sd, x, valid, dates, g


def paths(L, row, T, p, with_emb):
    nh, dm, _, _ = dims(row)
    d = L.LtaeDesc(row["B"], T, row["C"], row["h"] * row["w"], nh, dm, 1e-5, p, 0, None, None)
    f, b = ctypes.c_int(), ctypes.c_int()
    rc = L.lib().c2s_ltae_paths(ctypes.byref(d), int(with_emb), ctypes.byref(f), ctypes.byref(b))
    opt = L.lib().c2s_ltae_attn_optional(ctypes.byref(d))
    return rc, f.value, b.value, opt


def run_row(row, C_F):
    from crop2seg_amd import _lib as L
    from crop2seg_amd import engine as E
    from test_ops_gpu import make_ctx
    nh, dm, dk, dv = dims(row)
    with_emb, drop, p = row["emb"], row.get("drop", "none"), row.get("p", 0.0)
    res = {"row": row["name"]}
    if row["T"] == "max":       # the longest series whose tiles fit the LDS; one step more is a C-ABI error, not a launch
        fits = [t for t in range(1, 65) if paths(L, row, t, p, with_emb)[0] == 0]
        row = dict(row, T=max(fits))
        res["T"] = row["T"]
        assert fits == list(range(1, row["T"] + 1)), fits
        assert paths(L, row, row["T"] + 1, p, with_emb)[0] != 0
    B, T, C, h, w = row["B"], row["T"], row["C"], row["h"], row["w"]
    HW = h * w
    rc, fwd, bwd, opt = paths(L, row, T, p, with_emb)
    assert rc == 0 and [fwd, bwd] == row["want"], (row, rc, fwd, bwd)
    if (nh, dm) != (16, 256):
        assert opt == 0, "attn is never optional on the tile family"
    res.update(fwd=fwd, bwd=bwd)
    sd, x, valid, dates, g = inputs(row)
    keep = (torch.rand(nh, B * HW, T, generator=g) >= p).float() if drop == "keep" else None
    g_emb = torch.randn(B, dm, HW, generator=g) if with_emb else None
    g_attn = torch.randn(nh, B, T, HW, generator=g)
    xd = x.cuda()
    ctx = make_ctx(sd, training=True)
    priors = {}
    if row.get("acc"):                       # sinks that already hold a gradient: the block must add to them
        for k in FOLD + ["te.in_norm.weight", "te.in_norm.bias"] + [k for k in sd if ".positional_encoder" in k]:
            ctx.grad_sink(k)
            priors[k] = torch.randn(ctx.g[k].shape, generator=g)
            ctx.g[k].copy_(priors[k])
    emb, attn = E.ltae_attention(ctx, xd, dates.cuda(), valid.int().view(-1).cuda(), "te", nh, dk, dm, 1000.0, p, with_emb,
                                 row.get("rng_seed", 77), None if keep is None else keep.cuda(), pe_mode=row.get("pe", "rel"))
    assert attn is not None and tuple(attn.shape) == (nh, B, T, h, w)
    assert (emb is None) == (not with_emb) and (emb is None or tuple(emb.shape) == (B, dm, h, w))
    if emb is not None:
        ctx.tape.grads[emb.data_ptr()] = g_emb.cuda()
    ctx.tape.grads[attn.data_ptr()] = g_attn.view(attn.shape).cuda()
    ctx.tape.backward()
    torch.cuda.synchronize()
    gx = ctx.tape.grads[xd.data_ptr()].cpu()
    grads = {k: v.cpu() for k, v in ctx.g.items()}
    emb, attn = (None if emb is None else emb.cpu()), attn.cpu()
    if drop == "keep":
        mask = (keep.view(nh, B, HW, T).permute(0, 1, 3, 2) / (1.0 - p)).double()
    elif drop == "rng":
        # the counter-hash mask, recovered: dropped <=> exactly 0 at a valid position (attn_pre > 0 there, asserted below);
        # the backward kernels draw it again from the same counters, so a different mask there fails d x and the sums
        _, scale = thr_scale(p)
        a4 = attn.view(nh, B, T, HW)
        mask = (a4 != 0).double() * scale
        kept = ((a4 != 0) & valid[None, :, :, None])
        rate = 1.0 - float(kept.sum()) / float(valid.sum() * nh * HW)
        assert abs(rate - p) <= 6 * math.sqrt(p * (1 - p) / float(valid.sum() * nh * HW)), rate
        res["mask_crc"] = zlib.crc32(kept.numpy().tobytes())
    else:
        mask = None
    pe_mode = row.get("pe", "rel")
    if pe_mode == "rel":
        pe, A_pe = H.sinusoid_table(dates, nh, dv)
        pnames = {}
    else:                                        # learnable encoders: 16 / 256 only, any d_k (tests/ltae_ref.py has their tables)
        pnames = {k: v for k, v in ENC.items() if v + ".weight" in sd}
        pe, A_pe = R.pe_table(pe_mode, dates, {f"{k}.{s}": sd[f"{v}.{s}"] for k, v in pnames.items() for s in ("weight", "bias")})
    pix = H.pixel_subset(B, HW, n_random=16, seed=row.get("seed", 3))
    ref, A = H.ltae_hp_ref(x.view(B, T, C, HW), valid, H.params_of(sd, nh, dk, dv), pe, nh, dk, dv, A_pe, mask, g_emb, g_attn,
                           pixels=pix)
    if drop == "rng":
        assert bool((ref["attn_pre"].permute(0, 2, 1)[valid[pix // HW]] > 0).all()), "attn_pre underflows at a valid frame"
    b_idx, s_idx = pix // HW, pix % HW

    def check(name, got, key, frob, prior=None):
        r_, a_ = ref[key], A[key]
        c = C_F[name]
        if prior is not None:
            # accumulated: the gradient's own error, c u A as without a prior, and ONE float32 rounding of prior + gradient,
            # u |sum|, which no float32 accumulation can avoid (c < 1: at the small pixel counts of these rows A is a fraction
            # of |prior| and c u (A + |prior|), the form of tests/ltae_ref_worker.py, would ask for less than half an ulp of
            # the stored sum).  As A: c u (A + |sum| / c).  The same gradients are held to c u A alone by the row of the same
            # shape and hyper-parameters without a prior; the ratio under the older form is reported next to this one
            # ("<name>@old", not asserted), for the default hyper-parameters too (row default_acc).
            r_ = r_ + prior.double().view(r_.shape)
            old = (got.detach().double().cpu() - r_).abs() / (conv_ref.U * (a_ + prior.double().abs().view(r_.shape)) + 1e-30)
            res[name + "@old"] = float(old.max())
            a_ = a_ + r_.abs() / c
        res[name] = conv_ref.assert_within(f"{row['name']}: {name}", got, r_, a_, c, frob)

    check("attn", attn.view(nh, B, T, HW)[:, b_idx, :, s_idx], "attn", FROB["attn"])
    if emb is not None:
        check("emb", emb.view(B, dm, HW)[b_idx, :, s_idx], "emb", FROB["emb"])
    check("gx", gx.view(B, T, C, HW)[b_idx, :, :, s_idx], "gx", 1e-4)
    pr = priors.get
    # without the embedding, beta and bc only shift every score of a head alike: their gradients are 0 up to rounding, like
    # gbk always -- no Frobenius bar there, the per-element bound still holds (tests/ltae_ref_worker.py)
    zero = math.inf if not with_emb else 1e-4
    check("dgamma", grads["te.in_norm.weight"], "dgamma", 1e-4, pr("te.in_norm.weight"))
    check("dbeta", grads["te.in_norm.bias"], "dbeta", zero, pr("te.in_norm.bias"))
    check("gQ", grads["te.attention_head.Q"].view(nh, dk), "gQ", 1e-4, pr("te.attention_head.Q"))
    check("gWk", grads["te.attention_head.fc1_k.weight"], "gWk", 1e-4, pr("te.attention_head.fc1_k.weight"))
    check("gbk", grads["te.attention_head.fc1_k.bias"], "gbk", math.inf, pr("te.attention_head.fc1_k.bias"))
    check("gWc", grads["te.inconv.weight"].view(dm, C), "gWc", 1e-4, pr("te.inconv.weight"))
    check("gbc", grads["te.inconv.bias"], "gbc", zero, pr("te.inconv.bias"))
    if pnames:
        gp, Ap = R.pe_param_grads(pe_mode, dates, ref["gpe"], A["gpe"], {})
        for k, v in gp.items():
            full = ENC[k.split(".")[0]] + "." + k.split(".")[1]
            ref[k], A[k], C_F[k] = v, Ap[k], C_F["pe"]
            check(k, grads[full], k, 1e-4, pr(full))
    return res


def fold_same(row):
    """At 16 / 256 / 4 the _ex entry points of the parameter fold and the original ones give the same bits: U, s0, qwk of the
    forward, the five gradients of the adjoint (overwritten and accumulated), and the positional table."""
    from crop2seg_amd import _lib as L
    lib = L.lib()
    nh, dm, dk, dv = dims(row)
    B, T, C = row["B"], row["T"], row["C"]
    sd, _, _, dates, g = inputs(row)
    dev = torch.device("cuda")
    Q, Wk, bk, Wc, bc = (sd[k].to(dev).contiguous() for k in FOLD)
    dl = dates.cuda().contiguous()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()      # noqa: E731
    out = []
    for ex in (False, True):
        pe = torch.empty(B, T, dv, device=dev)
        U, s0, qwk = torch.empty(nh, C, device=dev), torch.empty(B, T, nh, device=dev), torch.empty(nh, dm, device=dev)
        if ex:
            assert lib.c2s_positional_table_ex(ptr(dl), ptr(pe), dl.numel(), 1000.0, dv, st) == 0
            assert lib.c2s_ltae_fold_fwd_ex(ptr(Q), ptr(Wk), ptr(bk), ptr(Wc), ptr(bc), ptr(pe), ptr(U), ptr(s0), ptr(qwk), B * T,
                                            C, nh, dk, dm, st) == 0
            nws = lib.c2s_ltae_fold_bwd_workspace_floats_ex(nh, dm)
        else:
            assert lib.c2s_positional_table(ptr(dl), ptr(pe), dl.numel(), 1000.0, st) == 0
            assert lib.c2s_ltae_fold_fwd(ptr(Q), ptr(Wk), ptr(bk), ptr(Wc), ptr(bc), ptr(pe), ptr(U), ptr(s0), ptr(qwk), B * T, C,
                                         st) == 0
            nws = lib.c2s_ltae_fold_bwd_workspace_floats()
        gg = torch.Generator().manual_seed(11)
        gU, gs0 = torch.randn(nh, C, generator=gg).cuda(), torch.randn(B, T, nh, generator=gg).cuda()
        gWc_a, gbc_a = torch.randn(dm, C, generator=gg).cuda(), torch.randn(dm, generator=gg).cuda()
        ws = torch.empty(nws, device=dev)
        got = [pe, U, s0, qwk]
        for acc_mask in (0, 31):
            sinks = [torch.randn(t.shape, generator=gg).cuda() for t in (Q, Wk, bk, Wc, bc)]
            args = [ptr(Q), ptr(Wk), ptr(bk), ptr(Wc), ptr(bc), ptr(pe), ptr(qwk), ptr(gU), ptr(gs0), ptr(gWc_a), ptr(gbc_a),
                    *[ptr(t) for t in sinks], B * T, C]
            if ex:
                assert lib.c2s_ltae_fold_bwd_ex(*args, nh, dk, dm, acc_mask, ptr(ws), ws.numel(), st) == 0
            else:
                assert lib.c2s_ltae_fold_bwd(*args, acc_mask, ptr(ws), ws.numel(), st) == 0
            got += sinks
        torch.cuda.synchronize()
        out.append([t.cpu() for t in got])
    assert lib.c2s_ltae_fold_bwd_workspace_floats_ex(16, 256) == lib.c2s_ltae_fold_bwd_workspace_floats()
    names = ["pe", "U", "s0", "qwk"] + [f"{k} acc={a}" for a in (0, 1) for k in ("gQ", "gWk", "gbk", "gWc", "gbc")]
    for n, a, b in zip(names, *out):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), n
    # outside the built set: an error code, no launch
    assert lib.c2s_ltae_fold_fwd_ex(ptr(Q), ptr(Wk), ptr(bk), ptr(Wc), ptr(bc), ptr(pe), ptr(U), ptr(s0), ptr(qwk), B * T, C, nh, 33,
                                    dm, st) != 0
    return {"row": row["name"], "same": len(names)}


def main():
    rows = json.loads(sys.argv[1])
    C_F = json.loads(sys.argv[2])
    arena_mib = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    for row in rows:
        res = run_row_in_arena(run_row, row, C_F, arena_mib) if arena_mib else run_row(row, C_F)
        if row.get("fold_same"):
            res.update(fold_same(row))
        print("ROW " + json.dumps(res), flush=True)
    print("LTAE_HP_OK", len(rows), flush=True)


if __name__ == "__main__":
    main()
