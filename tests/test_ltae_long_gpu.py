"""The time-chunked L-TAE family (csrc/ltae_long.hip: series longer than 64 steps, or every shape under C2S_LTAE_LONG=1)
against the float64 reference of tests/ltae_ref.py, element by element, with the constants of test_ltae_reference_gpu.py.

test_long_rows: T from 65 to 256, C in {64, 128, 256}, with and without the embedding and g_attn, explicit keep masks and the
counter hash at p = 0.1 / 0.5, accumulating sinks, a learnable positional encoder, maps that are not a multiple of the 64-pixel
tile, and one map that fills the chip at T = 72.  The worker's Frobenius bar on attn (2e-6) was set for T <= 64: on one
long series alone (B = 1) it is exceeded from about T = 190 on (2.9e-6 at T = 192, 4.4e-6 at T = 366) while every element
stays within its bound c u A (worst ratio 0.03 of 1); the rows past T = 129 therefore carry a second batch element, the
worker's one-valid-frame series, as every B = 2 row does.

test_forced_rows_draw_the_same_mask: every row of test_ltae_reference_gpu.rows_default() (T <= 64) through the long family
(C2S_LTAE_LONG=1); the rows with the RNG mask also run under the default switches, and the two processes must give the same
zero pattern (mask CRC): the long family draws the dropout of every other family.

test_timeunet_t72_hipgraph_replay_equals_eager: a TimeUNet train step at T = 72 (the L-TAE at full resolution through the long
family) replayed as a captured hipGraph is bit-identical to eager launches."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import ltae_ref as R
import test_ltae_reference_gpu as TG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG = [4, 6]


def rows_long():
    hf = TG.side(1, 64)          # 64 pixels per CU: the 64-pixel tiles fill the chip
    return [
        dict(name="t65_c64_hw32", B=2, T=65, C=64, h=4, w=8, emb=True, pad=True, want=LONG),
        dict(name="t72_c128_sharp", B=2, T=72, C=128, h=8, w=12, emb=True, pad=True, kind="sharp", want=LONG),
        dict(name="t129_c256_offset", B=1, T=129, C=256, h=4, w=4, emb=True, pad=True, kind="offset", want=LONG),
        dict(name="t256_c64_noemb", B=2, T=256, C=64, h=8, w=8, emb=False, pad=True, want=LONG),
        dict(name="t192_c64", B=2, T=192, C=64, h=8, w=8, emb=True, pad=True, want=LONG),
        dict(name="t200_c128_nogattn", B=2, T=200, C=128, h=4, w=4, emb=True, pad=True, need_attn=False, want=LONG),
        dict(name="t80_keep_p0.5", B=2, T=80, C=64, h=4, w=8, emb=True, pad=True, p=0.5, want=LONG),
        dict(name="rng_t81_p0.1", B=2, T=81, C=64, h=8, w=8, emb=True, pad=True, drop="rng", p=0.1, want=LONG),
        dict(name="rng_t97_c128_p0.5", B=1, T=97, C=128, h=8, w=8, emb=True, pad=True, drop="rng", p=0.5, want=LONG),
        dict(name="acc_abs_rel_doy_t70", B=1, T=70, C=128, h=4, w=4, emb=True, pad=True, acc=True, pe="abs_rel_doy", want=LONG),
        dict(name="acc_t68", B=2, T=68, C=64, h=4, w=4, emb=True, pad=True, acc=True, want=LONG),
        dict(name="fill_t72_rng", B=1, T=72, C=64, h=hf, w=hf, emb=True, pad=True, drop="rng", p=0.1, want=LONG),
    ]


def run_worker(rows, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ltae_ref_worker.py"), json.dumps(rows), json.dumps(R.C_KERNEL)],
                       env=env, capture_output=True, text=True, timeout=1200)
    res = {}
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            d = json.loads(line[4:])
            print(d)
            res[d["row"]] = d
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert f"LTAE_REF_OK {len(rows)}" in r.stdout
    return res


def test_long_rows():
    res = run_worker(rows_long(), {})
    assert {(v["fwd"], v["bwd"]) for v in res.values()} == {tuple(LONG)}


def test_forced_rows_draw_the_same_mask():
    base = TG.rows_default()
    forced = [dict(r, want=LONG) for r in base]
    got = run_worker(forced, {"C2S_LTAE_LONG": "1"})
    rng = [r for r in base if r.get("drop") == "rng"]
    assert rng
    ref = run_worker(rng, {})
    for r in rng:
        assert got[r["name"]]["mask_crc"] == ref[r["name"]]["mask_crc"], r["name"]


def test_timeunet_t72_hipgraph_replay_equals_eager():
    import gc
    from crop2seg_amd import _lib
    from crop2seg_amd.learning import utils as LU
    from crop2seg_amd.learning.synthetic import synthetic_batch
    from oracle import seeded
    import ctypes
    B, T, H = 1, 72, 32
    d = _lib.LtaeDesc(B, T, 64, H * H, 16, 256, 1e-5, 0.0, 0, None, None)
    assert _lib.lib().c2s_ltae_fwd_path(ctypes.byref(d)) == 4
    x, dates, y, _ = synthetic_batch(B, T, H, H, 3, "cuda", irregular=False, lengths=[T - 5])

    def fresh():
        torch.manual_seed(3)
        net = LU.get_model(LU.default_config("timeunet"))
        ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        net.load_state_dict(seeded.make_state(ks, 41, "tame"))
        net = net.cuda().train()
        net.spec.attn_dropout = 0.0
        net.spec.mlp_dropout = 0.0
        return net, LU.TrainStep(net, num_classes=15)

    net_e, step_e = fresh()
    for _ in range(3):
        loss_e, _ = step_e(x, dates, y)
    torch.cuda.synchronize()
    loss_e, param_e = float(loss_e), step_e.flat_param.clone()
    assert step_e.ws.sync_error() == 0
    del net_e, step_e
    gc.collect()
    torch.cuda.empty_cache()
    net_g, step_g = fresh()
    step_g(x, dates, y)
    step_g.capture(x, dates, y)
    for _ in range(2):
        loss_g, _ = step_g.replay()
    torch.cuda.synchronize()
    assert math.isfinite(loss_e) and float(loss_g) == loss_e
    assert torch.equal(step_g.flat_param, param_e)
    assert step_g.ws.sync_error() == 0
