"""engine.ltae_attention on maps whose pixel count is no multiple of 4, against the CPU oracle.

The L-TAE kernels walk a sample's pixels four at a time and refuse other maps ("ltae: h*w must be a multiple of 4").  Every
test map was square with an even side, so nothing noticed that U-TAE and W-TAE, whose L-TAE sees the H/8 x W/8 map, failed
with that C-ABI error in the forward on inputs that _check_inputs accepts: 24 x 24 (3 x 3), 16 x 24 (2 x 3), 24 x 40
(3 x 5) ...  engine.ltae_attention now runs such a map as the row of its pixels followed by zero pixels
(test_models_rect_gpu.py holds the whole models at 24 x 24 and 16 x 24).  Here the op itself, forward and backward, at the
bars of test_ops_gpu.test_ltae_attention_fwd_bwd: attention within max(3 x the fp32 oracle's own error against fp64, 2e-6),
embedding within max(3 x its error, 1e-5) relative, d x within 1e-4 relative, every parameter gradient within
1e-4 |ref| + 1e-6 gmax -- the last is what fails if the added pixels leak into a sum over pixels.  Maps: 3 x 3, 2 x 3, 3 x 5 and
1 x 7 (1, 2, 1 and 1 added pixels) at C = 128 (U-TAE) and 64 (W-TAE), with a padded frame, with and without the embedding,
and with a prior gradient on x (the slice of the padded gradient is ADDED to it)."""
import pytest
import torch

from test_ops_gpu import O, _engine, _ltae_state, make_ctx, rel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,T,C,h,w,with_emb", [
    (2, 6, 128, 3, 3, True), (2, 4, 128, 2, 3, True), (1, 5, 64, 3, 5, True), (2, 7, 64, 1, 7, True), (2, 6, 64, 3, 3, False),
])
def test_ltae_attention_odd_map_fwd_bwd(B, T, C, h, w, with_emb):
    E, L = _engine()
    assert (h * w) % 4 != 0
    g = torch.Generator().manual_seed(13)
    sd = _ltae_state(C, g)
    cfg = O.BackboneConfig()
    x = torch.randn(B, T, C, h, w, generator=g)
    dates = (5 * torch.arange(T)[None] + torch.arange(B)[:, None]).long()
    valid = torch.ones(B, T, dtype=torch.int32)
    valid[0, T - 2:] = 0
    x[0, T - 2:] = 0
    dates[0, T - 2:] = 0
    x.requires_grad_(True)
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    emb, attn = O.ltae_attention(x, dates, ~valid.bool(), sdg, "te", cfg, None)
    attn5 = attn.view(16, B, h, w, T).permute(0, 1, 4, 2, 3)
    emb4 = emb.view(B, h, w, 256).permute(0, 3, 1, 2)
    g_attn = torch.randn(attn5.shape, generator=g)
    g_emb = torch.randn(emb4.shape, generator=g)
    prior = torch.randn(x.shape, generator=g)
    loss = (attn5 * g_attn).sum() + ((emb4 * g_emb).sum() if with_emb else 0)
    loss.backward()

    ctx = make_ctx({k: v for k, v in sd.items()}, training=True)
    xd = x.detach().cuda()
    ctx.tape.grads[xd.data_ptr()] = prior.cuda()
    e_out, a_out = E.ltae_attention(ctx, xd, dates.cuda(), valid.view(-1).cuda(), "te", 16, 4, 256, 1000.0, 0.0, with_emb, 0, None)
    assert a_out.shape == (16, B, T, h, w) and a_out.is_contiguous()
    assert (e_out is None) == (not with_emb)
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        emb64, attn64 = O.ltae_attention(x.detach().double(), dates, ~valid.bool(), sd64, "te", cfg, None)
    a64 = attn64.view(16, B, h, w, T).permute(0, 1, 4, 2, 3)
    e64 = emb64.view(B, h, w, 256).permute(0, 3, 1, 2)
    a_err32 = float((attn5.detach().double() - a64).abs().max())
    assert float((a_out.cpu().double() - a64).abs().max()) <= max(3 * a_err32, 2e-6)
    assert float(a_out[:, 0, T - 2:].abs().max()) == 0.0, "padded frames get exactly zero attention"
    if with_emb:
        assert e_out.shape == (B, 256, h, w) and e_out.is_contiguous()
        assert rel(e_out, e64) <= max(3 * rel(emb4, e64), 1e-5)
        ctx.tape.grads[e_out.data_ptr()] = g_emb.cuda().contiguous()
    ctx.tape.grads[a_out.data_ptr()] = g_attn.cuda().contiguous()
    ctx.tape.backward()
    torch.cuda.synchronize()
    assert rel(ctx.tape.grads[xd.data_ptr()], x.grad + prior) < 1e-4
    gmax = max(float(v.grad.norm()) for v in sdg.values())
    for k, v in sdg.items():
        assert float((ctx.g[k].cpu() - v.grad).norm()) <= 1e-4 * float(v.grad.norm()) + 1e-6 * gmax, k
