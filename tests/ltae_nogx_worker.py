"""Child process of tests/test_frozen_gpu.py: the L-TAE backward without the input gradient (c2s_ltae_attn_bwd with gx == NULL,
and with ggamma == gbeta == NULL as well) against the full call, through the engine, in a process whose environment selects
the kernel path (the dispatch switches of csrc/ltae.hip are read once per process).  Case: B,T,C,h,with_emb,pad,drop,
need_attn,expected backward path.  Prints LTAE_NOGX_OK when every parameter output is bit-identical."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run(sd, x, dates, valid, p_drop, with_emb, need_attn, trainable, g_emb, g_attn):
    import torch
    from crop2seg_amd import engine as E
    dev = torch.device("cuda")
    p = {k: v.to(dev).contiguous() for k, v in sd.items()}
    names = list(p) if trainable is None else trainable
    grads = {k: torch.full_like(p[k], float("nan")) for k in names}
    ctx = E.Ctx(p, {}, grads, E.Workspace(dev), True, E.Tape(), trainable=trainable)
    emb, attn = E.ltae_attention(ctx, x, dates, valid, "te", 16, 4, 256, 1000.0, p_drop, with_emb, 1234, None, None,
                                 need_attn=need_attn)
    if emb is not None:
        ctx.tape.grads[emb.data_ptr()] = g_emb.clone()
    if attn is not None:
        ctx.tape.grads[attn.data_ptr()] = g_attn.clone()
    ctx.tape.backward()
    torch.cuda.synchronize()
    return grads, attn is None


def main():
    import torch
    from crop2seg_amd import _lib
    from test_ops_gpu import _ltae_state
    cases = [[int(v) for v in c.split(",")] for c in sys.argv[1:]]
    for B, T, Cc, h, with_emb, pad, drop, need_attn, path in cases:
        g = torch.Generator().manual_seed(13)
        sd = _ltae_state(Cc, g)
        x = torch.randn(B, T, Cc, h, h, generator=g)
        dates = (5 * torch.arange(T)[None] + torch.arange(B)[:, None]).long()
        valid = torch.ones(B, T, dtype=torch.int32)
        if pad:
            valid[0, T - 2:] = 0
            x[0, T - 2:] = 0
            dates[0, T - 2:] = 0
        g_emb = torch.randn(B, 256, h, h, generator=g).cuda()
        g_attn = torch.randn(16, B, T, h, h, generator=g).cuda()
        x, dates, valid = x.cuda(), dates.cuda(), valid.view(-1).cuda()
        p_drop = 0.1 if drop else 0.0
        d = _lib.LtaeDesc(B, T, Cc, h * h, 16, 256, 1e-5, p_drop, 1234, None, None)
        if not need_attn and _lib.lib().c2s_ltae_attn_optional(C.byref(d)):
            d.keep_bits = x.data_ptr()              # any non-NULL pointer: the query only tests it
        fwd, bwd = C.c_int(), C.c_int()
        assert _lib.lib().c2s_ltae_paths(C.byref(d), int(with_emb), C.byref(fwd), C.byref(bwd)) == 0
        assert bwd.value == path, (B, T, Cc, h, "backward path", bwd.value, "expected", path)
        args = (x, dates, valid, p_drop, bool(with_emb), bool(need_attn))
        full, no_attn = run(sd, *args, None, g_emb, g_attn)
        assert no_attn == (path == 4)
        every = [k for k in sd]
        fold = [k for k in sd if ".in_norm." not in k]
        for trainable in (every, fold):          # gx == NULL; gx == ggamma == gbeta == NULL
            got, _ = run(sd, *args, trainable, g_emb, g_attn)
            for k in trainable:
                assert torch.equal(got[k], full[k]), (B, T, Cc, h, path, len(trainable), k)
        print("case", B, T, Cc, h, "path", path, "ok", flush=True)
    print("LTAE_NOGX_OK", len(cases))


if __name__ == "__main__":
    main()
