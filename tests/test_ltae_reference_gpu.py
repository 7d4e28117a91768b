"""Every L-TAE kernel family of csrc/ltae.hip against the float64 reference of tests/ltae_ref.py, element by element, and the
counter-hash dropout that training uses.

The op test (test_ops_gpu.py::test_ltae_attention_fwd_bwd) holds the gradients to one Frobenius bar of 1e-4 and always passes
an explicit keep mask.  Here every row (tests/ltae_ref_worker.py, one child process per set of C2S_LTAE_* switches: they are
read once per process) checks attn, emb, gx on every frame of a pixel subset (padded frames included), and the parameter
gradients d gamma, d beta, d Q, d fc1_k, d inconv and those of the learnable positional encoders, summed over every pixel,
against |got - ref| <= c * u * A (u = 2^-24, A = first-order rounding propagation, tests/ltae_ref.py) next to the Frobenius
bars of test_ops_gpu.py.  Each row asserts the forward / backward families it reached (c2s_ltae_paths) and
test_reached_families_are_the_table asserts the union.  Rows with the RNG mask recover it from attn (dropped <=> exactly 0
at a valid frame) and run the reference with it: the forward and the backward family must draw the same mask.

Not run per element: the B = 9 / B = 17 size fallbacks of test_ltae_paths_gpu.py (x alone 9.2 / 17.4 GB: the float64
reference of the parameter sums would need several times that in host memory); the families they select -- register-resident
forward with streaming heads + gx64, and the three-pass streaming pair -- are reached here through the switches on smaller
batches.  ltae_reg_fwd_kernel<false> (more than 2^32 dropout counters, x of about 136 GB) stays unreached.

Error constants c: about 4x the worst ratio observed on an MI355X (printed with -s).  Observed worst ratios:

    family              attn    emb     gx       dgamma   dbeta    gQ       gWk      gbk      gWc      gbc      pe enc.
    reg (fwd)           0.022   0.19
    stream (fwd)        0.023   0.30
    lds (fwd)           0.024   0.21
    16-pixel (fwd)      0.024   0.17
    reg<false>+gx64                     6.4e-4   5.6e-7   4.4e-7   2.7e-5   4.7e-5   1.4e-5   4.2e-5   5.6e-6   5.6e-6
    reg<true>+gx64                      3.6e-4   4.5e-7   3.9e-7   1.4e-5   3.5e-5   7.4e-6   3.1e-5   5.7e-6
    stream+gx64                         3.9e-4   5.2e-7   2.8e-7   1.6e-5   3.9e-5   1.3e-5   4.2e-5   3.5e-6
    stream+gx4                          1.9e-4   4.4e-7   3.0e-7   1.3e-5   3.4e-5   5.0e-6   4.4e-5   2.9e-6
    lds (bwd)                           3.8e-4   1.5e-5   1.3e-5   7.8e-4   4.7e-3   2.3e-4   6.3e-4   9.9e-5   2.2e-4
    8-pixel                             4.8e-4   1.7e-5   1.1e-5   4.9e-4   1.1e-3   1.9e-4   4.3e-4   9.0e-5

The constants (tests/ltae_ref.py C_KERNEL) are per output: attn 0.1, emb 1.2, gx 0.003, d gamma / d beta 1e-4, gQ 0.004,
gWk 0.02, gbk 0.001, gWc 0.003, gbc 5e-4, encoders 0.001.  The ratios of the parameter sums sit far below 1: A adds |terms|
over every pixel while the sums cancel, so there the Frobenius bar of 1e-4 stays the sharper check of a lost partial; the
per-element bound catches a wrong element or channel row.

Found by these rows: with an explicit keep mask the engine held the mask only through the descriptor's raw pointer, so a
caller that let go of its tensor after the forward made the 8-pixel, streaming-heads and gx<4> backward kernels read freed
memory (reg_hw16_not64, stream_t39, reg_fwd_stream_bwd_t9, px16_c64_t9 failed with d x 10-20 % off); engine.ltae_attention
now keeps the mask on the tape.  The register-resident backward reads attn, not the mask, and was unaffected.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import ltae_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_F = R.C_KERNEL
FWD = {0: "16-pixel", 1: "stream", 2: "reg", 3: "lds"}
BWD = {0: "8-pixel", 1: "stream+gx4", 2: "stream+gx64", 3: "reg<false>+gx64", 4: "reg<true>+gx64", 5: "lds"}
REACHED = set()
OBSERVED = {}
CRC = {}


def cus():
    from crop2seg_amd import _lib
    return _lib.lib().c2s_device_cus()


def side(B, per_cu):
    """Square side (multiple of 8) with B * side^2 >= per_cu * CUs pixels: 64 per CU fill the register-resident tiles four
    times over (16-pixel tiles, >= 4 per CU), 128 per CU the streaming kernels' 64-pixel tiles twice."""
    return 8 * math.ceil(math.sqrt(per_cu * cus() / B) / 8)


def rows_default():
    h1, h2, h3, hf = side(1, 64), side(2, 128), side(3, 128), side(1, 128)
    h4 = side(2, 128)
    h4 += 4 if (h4 * h4) % 64 == 0 else 0            # h = 4 (mod 8): h*h a multiple of 16, not of 64
    Bs = max(1, math.ceil(2 * cus() / 512))          # 180 x 182: multiple of 8 pixels, not of 16 -> streaming forward
    r = [
        dict(name="reg_t61", B=1, T=61, C=64, h=hf, w=hf, emb=True, pad=True, want=[2, 3]),
        dict(name="reg_offset_t9_ragged", B=3, T=9, C=64, h=h3, w=h3, emb=True, pad=True, kind="offset", want=[2, 3]),
        dict(name="reg_sharp_t8", B=2, T=8, C=64, h=h2, w=h2, emb=True, pad=True, kind="sharp", want=[2, 3]),
        dict(name="reg_hw16_not64", B=2, T=7, C=64, h=h4, w=h4, emb=True, pad=True, want=[2, 1]),
        dict(name="stream_hw8_t13", B=Bs, T=13, C=64, h=180, w=182, emb=True, pad=True, want=[1, 1]),
        dict(name="reg_fwd_lds_bwd_noemb", B=1, T=7, C=64, h=h1, w=h1, emb=False, pad=True, want=[2, 5]),
        dict(name="lds_c128_t39", B=2, T=39, C=128, h=8, w=8, emb=True, pad=True, kind="sharp", want=[3, 5]),
        dict(name="px16_c256_t31_hw20", B=1, T=31, C=256, h=4, w=5, emb=True, pad=True, want=[0, 0]),
        dict(name="lds_c256_t9", B=2, T=9, C=256, h=4, w=4, emb=True, pad=True, kind="sharp", want=[3, 5]),
        dict(name="lds_fwd_8px_bwd_c128_t48", B=1, T=48, C=128, h=4, w=4, emb=True, pad=True, want=[3, 0]),
        dict(name="px16_fwd_c256_t39", B=2, T=39, C=256, h=4, w=4, emb=True, pad=True, kind="offset", want=[0, 0]),
        dict(name="t1", B=2, T=1, C=64, h=4, w=4, emb=True, pad=False, want=[3, 5]),
        dict(name="t2_c128", B=2, T=2, C=128, h=4, w=4, emb=False, pad=True, want=[3, 5]),
        dict(name="t57_offset", B=1, T=57, C=64, h=4, w=8, emb=True, pad=True, kind="offset", want=[3, 5]),
        dict(name="t64", B=2, T=64, C=64, h=4, w=4, emb=True, pad=True, want=[3, 5]),
        dict(name="acc_abs_rel_doy", B=2, T=9, C=128, h=4, w=4, emb=True, pad=True, acc=True, pe="abs_rel_doy", want=[3, 5]),
        dict(name="acc_reg", B=1, T=8, C=64, h=hf, w=hf, emb=True, pad=True, acc=True, want=[2, 3]),
        dict(name="rng_reg_p0.1", B=2, T=9, C=64, h=h2, w=h2, emb=True, pad=True, drop="rng", p=0.1, want=[2, 3]),
        dict(name="rng_reg_p0.5", B=2, T=9, C=64, h=h2, w=h2, emb=True, pad=True, drop="rng", p=0.5, want=[2, 3]),
        dict(name="rng_reg_noattn_p0.5", B=2, T=9, C=64, h=h2, w=h2, emb=True, pad=True, drop="rng", p=0.5, need_attn=False,
             want=[2, 4]),
        dict(name="rng_reg_fwd_lds_bwd_noemb", B=1, T=7, C=64, h=h1, w=h1, emb=False, pad=True, drop="rng", p=0.5, want=[2, 5]),
        dict(name="rng_lds_p0.5", B=2, T=31, C=128, h=4, w=8, emb=True, pad=True, drop="rng", p=0.5, want=[3, 5]),
        dict(name="rng_lds_8px_p0.1", B=1, T=48, C=128, h=4, w=4, emb=True, pad=True, drop="rng", p=0.1, want=[3, 0]),
    ]
    for mode in ("doy", "abs_rel", "linear", "abs_rel_doy", "abs_rel_linear"):
        r.append(dict(name=f"pe_{mode}_small", B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, pe=mode, want=[3, 5]))
        r.append(dict(name=f"pe_{mode}_full", B=1, T=5, C=64, h=hf, w=hf, emb=True, pad=True, pe=mode, want=[2, 3]))
    return r


def rows_stream():
    h2 = side(2, 128)
    return [dict(name="stream_t39", B=2, T=39, C=64, h=h2, w=h2, emb=True, pad=True, want=[1, 2]),
            dict(name="rng_stream_p0.5", B=2, T=9, C=64, h=h2, w=h2, emb=True, pad=True, drop="rng", p=0.5, want=[1, 2])]


def rows_reg_fwd_stream_bwd():
    h2 = side(2, 128)
    return [dict(name="rng_reg_fwd_stream_bwd_p0.1", B=2, T=9, C=64, h=h2, w=h2, emb=True, pad=True, drop="rng", p=0.1,
                 want=[2, 2]),
            dict(name="reg_fwd_stream_bwd_t9", B=1, T=9, C=64, h=side(1, 128), w=side(1, 128), emb=True, pad=True,
                 want=[2, 2])]


def rows_no_lds():
    return [dict(name="px16_c64_t9", B=2, T=9, C=64, h=4, w=4, emb=True, pad=True, want=[0, 0]),
            dict(name="px16_c128_t31", B=1, T=31, C=128, h=8, w=8, emb=True, pad=True, kind="sharp", want=[0, 0]),
            dict(name="rng_px16_p0.5", B=2, T=8, C=64, h=4, w=8, emb=True, pad=True, drop="rng", p=0.5, want=[0, 0])]


GROUPS = {
    "default": ({}, rows_default),
    "stream": ({"C2S_LTAE_REG": "0", "C2S_LTAE_REG_BWD": "0"}, rows_stream),
    "reg_fwd_stream_bwd": ({"C2S_LTAE_REG_BWD": "0"}, rows_reg_fwd_stream_bwd),
    "no_lds": ({"C2S_LTAE_LDS": "0", "C2S_LTAE_LDS_BWD": "0"}, rows_no_lds),
}


@pytest.mark.parametrize("group", list(GROUPS))
def test_rows_per_element(group):
    env_extra, rows = GROUPS[group]
    env = dict(os.environ, **env_extra)
    rs = rows()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ltae_ref_worker.py"), json.dumps(rs), json.dumps(C_F)],
                       env=env, capture_output=True, text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            res = json.loads(line[4:])
            print(res)
            REACHED.add((res["fwd"], res["bwd"]))
            for k, v in res.items():
                if isinstance(v, float):
                    key = (FWD[res["fwd"]] if k in ("attn", "emb") else BWD[res["bwd"]], k)
                    OBSERVED[key] = max(OBSERVED.get(key, 0.0), v)
            if "mask_crc" in res:
                CRC[res["row"]] = res["mask_crc"]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert f"LTAE_REF_OK {len(rs)}" in r.stdout


def test_reached_families_are_the_table():
    """Every forward family but ltae_reg_fwd_kernel<false>, every backward family, and the mixed pairs the dispatch makes."""
    for k in sorted(OBSERVED):
        print("observed", k, round(OBSERVED[k], 3))
    fwd = {f for f, _ in REACHED}
    bwd = {b for _, b in REACHED}
    assert fwd == set(FWD), fwd
    assert bwd == set(BWD), bwd
    assert {(2, 5), (3, 0), (2, 2), (2, 1)} <= REACHED, REACHED


def test_every_forward_family_draws_the_same_mask():
    """Same descriptor and seed: the register-resident and the streaming forward give the same zero pattern."""
    assert "rng_reg_p0.5" in CRC and "rng_stream_p0.5" in CRC, CRC
    assert CRC["rng_reg_p0.5"] == CRC["rng_stream_p0.5"]


# ---- statistics of the counter-hash dropout (one process: no switch involved)

def _attn_rng(B, T, HW, p, seed, seed_dev=None):
    from crop2seg_amd import engine as E
    from test_ops_gpu import _ltae_state, make_ctx
    sd = _ltae_state(64, torch.Generator().manual_seed(13))
    h = int(math.isqrt(HW))
    x = torch.randn(B, T, 64, h, HW // h, generator=torch.Generator().manual_seed(5)).cuda()
    dates = (5 * torch.arange(T)[None] + torch.arange(B)[:, None]).long().cuda()
    valid = torch.ones(B * T, dtype=torch.int32, device="cuda")
    ctx = make_ctx(sd, training=True, tape=False)
    sdv = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64, device="cuda")
    _, a = E.ltae_attention(ctx, x, dates, valid, "te", 16, 4, 256, 1000.0, p, False, seed, None, seed_dev=sdv)
    torch.cuda.synchronize()
    return (a == 0).view(16, B, T, HW)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_rates(p):
    B, T, HW = 2, 10, 64 * 64
    thr = int(p * 65536 + 0.5)
    q = thr / 65536
    drop = _attn_rng(B, T, HW, p, 1234)

    def within(rate, n, expect, what):
        sigma = math.sqrt(expect * (1 - expect) / n)
        assert abs(rate - expect) <= 6 * sigma, (what, rate, expect, sigma)

    d = drop.double()
    within(float(d.mean()), d.numel(), q, "overall")
    for h in range(16):
        within(float(d[h].mean()), d[h].numel(), q, ("head", h))
    for t in range(T):
        within(float(d[:, :, t].mean()), d[:, :, t].numel(), q, ("t", t))
    for par in (0, 1):
        within(float(d[:, :, par::2].mean()), d[:, :, par::2].numel(), q, ("parity", par))
    for m in range(16):
        within(float(d[..., m::16].mean()), d[..., m::16].numel(), q, ("pixel mod 16", m))
    for b in range(B):
        within(float(d[:, b].mean()), d[:, b].numel(), q, ("batch", b))
    pair = (d[:, :, 0::2] * d[:, :, 1::2])                  # the two 16-bit halves of one hash
    within(float(pair.mean()), pair.numel(), q * q, "pair (2u, 2u+1)")
    again = _attn_rng(B, T, HW, p, 1234)
    assert torch.equal(drop, again), "same seed, different mask"
    agree = q * q + (1 - q) ** 2
    for other in (_attn_rng(B, T, HW, p, 1235), _attn_rng(B, T, HW, p, 1234 + (1 << 32)),
                  _attn_rng(B, T, HW, p, 1234, seed_dev=1)):
        same = (drop == other).double()
        assert not torch.equal(drop, other)
        within(float(same.mean()), same.numel(), agree, "seed pair agreement")
    s0 = _attn_rng(B, T, HW, p, 1234, seed_dev=0)
    s1 = _attn_rng(B, T, HW, p, 1234, seed_dev=1)
    within(float((s0 == s1).double().mean()), s0.numel(), agree, "seed_dev 0 / 1")


def test_mlp_dropout_rate_and_backward_mask():
    """c2s_dropout_nchw (the L-TAE MLP dropout, c2s_uniform): drop rate p within 6 sigma; the backward zeroes exactly the
    elements the forward dropped and scales the rest by the forward's 1 / (1 - p)."""
    from crop2seg_amd import engine as E
    from test_ops_gpu import make_ctx
    p = 0.3
    x = (torch.rand(4, 128, 32, 32, generator=torch.Generator().manual_seed(2)) + 0.5).cuda()
    ctx = make_ctx({}, training=True)
    y = E.dropout_nchw(ctx, x, p, 99, None)
    g = (torch.rand(x.shape, generator=torch.Generator().manual_seed(3)) + 0.5).cuda()
    ctx.tape.grads[y.data_ptr()] = g.clone()
    ctx.tape.backward()
    gx = ctx.tape.grads[x.data_ptr()]
    torch.cuda.synchronize()
    dropped = y == 0
    rate = float(dropped.double().mean())
    assert abs(rate - p) <= 6 * math.sqrt(p * (1 - p) / y.numel()), rate
    scale = y[~dropped] / x[~dropped]
    assert float((scale - 1 / (1 - p)).abs().max()) <= 1e-6
    assert torch.equal(gx == 0, dropped)
    assert float((gx[~dropped] / g[~dropped] - 1 / (1 - p)).abs().max()) <= 1e-6
