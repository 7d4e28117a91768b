"""The L-TAE at n_head in {8, 16}, d_model / n_head in {8, 16, 32} and d_k in 1..32, on the GPU.

Rows (tests/ltae_hp_worker.py, one child process): engine.ltae_attention forward and backward at the smallest shapes at which
each generalised piece of the 16-pixel forward / 8-pixel backward family can go wrong, against the float64 reference of
tests/ltae_hp_ref.py: attn, emb, gx on every frame of every pixel, d gamma, d beta, d Q, d fc1_k, d inconv summed over all
pixels; |got - ref| <= c * u * A with c = ltae_ref.C_KERNEL unchanged, next to the Frobenius bars of test_ops_gpu.py (1e-4 on
the gradients).  Every row asserts its families (c2s_ltae_paths): any (n_head, d_model) other than (16, 256) runs 0 / 0
whatever the map, a d_k other than 4 at (16, 256) keeps the default families (3 / 5 at these shapes).

    h8_dv32_partial   8 heads: half of the (pixel, head) threads idle; head width 32: two MFMA column blocks; HW = 20 leaves a
                      partial 16-pixel and a partial 8-pixel tile; C / n_head = 16; padded frames
    h8_dv16_c64       g_attn and g_emb both given (every row gives both where it has an embedding)
    h8_dv8_noemb      head width 8; W-TAE's emb == NULL; padded
    h16_dv8           head width 8 with masked MFMA columns in the forward; d_k = 1
    h16_dv32_t        the largest LDS tiles: T = 64 does not fit the 8-pixel backward's carve-up at C = 128 (173 056 bytes),
                      so the row runs the longest T that check() accepts (59) and asserts that T + 1 is a C-ABI error
    h8_keepmask       explicit keep mask [8,P,T], p = 0.5
    h8_rng            counter-hash mask, p = 0.5, recovered from attn: forward and backward draw the same mask
    dk6_lds           default families with d_k = 6
    dk32, dk32_acc    d_k = 32: without a prior under the unchanged bound, and accumulating into gradients that are already there
    default_acc       the shape of dk32_acc at 16 / 256 / 4: the yardstick of the accumulate rows
    dk6_pe_*, dk3_pe_*  a learnable positional encoder with d_k other than 4 (c2s_ltae_pe_bwd_ex: the encoders' share of d Q and
                      d fc1_k); the encoders' own gradients against tests/ltae_ref.pe_param_grads, constant C_KERNEL["pe"]
    default_same      16 / 256 / 4, and the _ex fold entry points against the original ones, bit for bit

Worst observed ratios |got - ref| / (u A) on an MI355X (the "16-pixel (fwd)" and "8-pixel" lines of
tests/test_ltae_reference_gpu.py are the yardstick at the default hyper-parameters):

    row                attn    emb     gx       dgamma   dbeta    gQ       gWk      gbk      gWc      gbc
    h8_dv32_partial    0.015   0.14    1.1e-4   1.4e-5   1.1e-5   4.3e-4   6.3e-4   1.2e-4   2.7e-4   6.8e-5
    h8_dv16_c64        0.022   0.019   4.3e-4   5.0e-5   4.6e-5   7.6e-4   1.5e-3   2.9e-4   9.0e-4   3.1e-4
    h8_dv8_noemb       0.034           3.8e-4   4.2e-5   1.2e-5   6.7e-4   1.5e-3   3.6e-4   3.0e-4   9.3e-5
    h16_dv8            0.040   0.15    6.8e-4   4.3e-5   2.0e-5   2.8e-4   2.9e-3   5.2e-4   8.2e-4   1.5e-4
    h16_dv32_t (T=59)  0.014   0.009   3.0e-4   4.6e-6   3.1e-6   3.6e-4   1.2e-3   1.8e-4   3.1e-4   8.0e-5
    h8_keepmask        0.019   0.17    7.7e-4   1.8e-5   1.7e-5   4.1e-4   1.1e-3   1.3e-4   4.7e-4   1.8e-4
    h8_rng             0.014   0.16    5.4e-4   2.9e-5   1.9e-5   6.9e-4   1.2e-3   1.8e-4   8.0e-4   1.5e-4
    dk6_lds            0.018   0.16    8.7e-5   8.2e-6   5.4e-6   3.9e-4   7.7e-4   1.0e-4   2.5e-4   5.4e-5
    dk32               0.006   0.19    3.1e-4   2.8e-5   1.9e-5   7.5e-4   1.3e-3   2.4e-4   1.4e-3   2.5e-4
    dk32_acc           0.006   0.19    3.1e-4   2.6e-5   2.2e-5   7.6e-4   1.4e-2   3.9e-4   1.3e-3   1.6e-4
      older form                                2.8e-5   2.3e-5   7.8e-4   7.5e-2   4.9e-4   1.4e-3   2.1e-4
    default_acc        0.016   0.15    1.4e-4   1.4e-5   8.2e-6   4.2e-4   6.3e-3   1.3e-4   4.3e-4   6.4e-5
      older form                                1.4e-5   8.5e-6   4.2e-4   9.6e-3   1.4e-4   4.4e-4   6.7e-5
    dk6_pe_abs_rel_li. 0.008   0.13    7.6e-5   9.0e-6   4.5e-6   4.9e-4   8.9e-4   1.8e-4   2.7e-4   3.7e-5   (encoders 1.6e-4)
    dk6_pe_.._acc      0.008   0.13    7.6e-5   9.0e-6   5.5e-6   4.9e-4   4.8e-3   2.0e-4   2.7e-4   4.1e-5   (encoders 2.5e-4)
      older form                                9.0e-6   5.6e-6   4.9e-4   5.8e-3   2.2e-4   2.7e-4   4.3e-5   (encoders 3.6e-4)
    dk3_pe_doy         0.013   0.14    2.6e-4   1.3e-5   1.1e-5   7.7e-4   1.5e-3   1.7e-4   6.1e-4   1.2e-4   (encoder 9.9e-5)
    default_same       0.013   0.14    1.2e-4   1.0e-5   7.3e-6   4.7e-4   1.1e-3   1.5e-4   3.9e-4   5.5e-5
    constant c         0.1     1.2     3e-3     1e-4     1e-4     4e-3     2e-2     1e-3     3e-3     5e-4

No row needs a constant of its own.  Every gradient is held to c u A alone by a row without a prior (dk32, dk6_pe_abs_rel_linear,
dk6_lds, ...).  The accumulate rows add a prior of N(0, 1) entries: their bound is c u A for the gradient plus u |sum| for the one
float32 rounding of prior + gradient (tests/ltae_hp_worker.py).  "older form" is the ratio against c u (A + |prior|), the form
of tests/ltae_ref_worker.py, reported and not asserted.  With 32 pixels A is a fraction of |prior|; at d_k = 32 fc1_k is
initialised with std sqrt(2 / 32) and d fc1_k.weight is smaller still, so c u (A + |prior|) asks for 0.02 ulp of the stored sum:
gWk stands at 0.075 there (81 of 131072 elements beyond 0.02, each by one rounding of the sum: got 2.382642031, ref 2.382641913,
u |sum| = 1.42e-7), against 0.0096 for default_acc, the same shape at d_k = 4.  Four times that yardstick (0.038) would not
cover it either: the miss is the float32 format's, not a constant's, and the row without a prior shows gWk at 1.3e-3 of c u A.

Whole models: the model classes open d_model alone (n_head and d_k stay at 16 / 4 there: tests/test_abi.py), so the rows above
reach n_head = 8 and the other d_k through engine.ltae_attention.  The fixture of tools/make_golden_ltae_hparams.py
(TimeUNet, d_model = 512) runs under the parity protocol of tests/test_models_gpu.py (which also picks it up by globbing, in both
convolution modes), and TimeUNet at d_model = 128 takes one TrainStep step.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import ltae_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["timeunet_eval_h16m512k4_tame"]

ROWS = [
    dict(name="h8_dv32_partial", nh=8, dm=256, dk=8, B=2, T=5, C=128, h=4, w=5, emb=True, pad=True, want=[0, 0]),
    dict(name="h8_dv16_c64", nh=8, dm=128, dk=2, B=1, T=9, C=64, h=4, w=4, emb=True, pad=False, want=[0, 0]),
    dict(name="h8_dv8_noemb", nh=8, dm=64, dk=3, B=2, T=7, C=64, h=4, w=4, emb=False, pad=True, want=[0, 0]),
    dict(name="h16_dv8", nh=16, dm=128, dk=1, B=2, T=6, C=64, h=4, w=5, emb=True, pad=True, want=[0, 0]),
    dict(name="h16_dv32_t", nh=16, dm=512, dk=4, B=1, T="max", C=128, h=4, w=4, emb=True, pad=True, want=[0, 0]),
    dict(name="h8_keepmask", nh=8, dm=256, dk=4, B=2, T=8, C=64, h=4, w=8, emb=True, pad=True, drop="keep", p=0.5,
         want=[0, 0]),
    dict(name="h8_rng", nh=8, dm=128, dk=4, B=2, T=8, C=64, h=4, w=8, emb=True, pad=True, drop="rng", p=0.5, want=[0, 0]),
    dict(name="dk6_lds", nh=16, dm=256, dk=6, B=2, T=9, C=128, h=4, w=4, emb=True, pad=True, want=[3, 5]),
    dict(name="dk32", nh=16, dm=256, dk=32, B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, want=[3, 5]),
    dict(name="dk32_acc", nh=16, dm=256, dk=32, B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, acc=True, want=[3, 5]),
    dict(name="dk6_pe_abs_rel_linear_acc", nh=16, dm=256, dk=6, B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, acc=True,
         pe="abs_rel_linear", want=[3, 5]),
    dict(name="dk6_pe_abs_rel_linear", nh=16, dm=256, dk=6, B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, pe="abs_rel_linear",
         want=[3, 5]),
    dict(name="default_acc", nh=16, dm=256, dk=4, B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, acc=True, want=[3, 5]),
    dict(name="dk3_pe_doy", nh=16, dm=256, dk=3, B=2, T=7, C=64, h=4, w=4, emb=True, pad=True, pe="doy", want=[3, 5]),
    dict(name="default_same", nh=16, dm=256, dk=4, B=2, T=9, C=64, h=4, w=4, emb=True, pad=True, fold_same=True,
         want=[3, 5]),
]


def test_rows_per_element():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ltae_hp_worker.py"), json.dumps(ROWS),
                        json.dumps(R.C_KERNEL)], capture_output=True, text=True, timeout=600)
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            res = json.loads(line[4:])
            print(res)
            seen[res["row"]] = res
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert f"LTAE_HP_OK {len(ROWS)}" in r.stdout
    assert set(seen) == {row["name"] for row in ROWS}
    assert seen["h16_dv32_t"]["T"] == 59            # (163840 / 4 - 2048 - 4096 - 4096 - 256) / (4 * 16 * 8) = 59.5
    assert seen["default_same"]["same"] == 14
    assert "emb" not in seen["h8_dv8_noemb"] and all("emb" in v for k, v in seen.items() if k != "h8_dv8_noemb")


@pytest.mark.parametrize("name", FIXTURES)
def test_model_matches_reference(goldens, name):
    """tests/test_models_gpu.py::test_model_matches_reference on the fixtures named here (f32 convolutions)."""
    import test_models_gpu as TM
    from crop2seg_amd import engine as E
    g = goldens(name)
    assert (g.ctor["n_head"], g.ctor["d_model"], g.ctor["d_k"]) != (16, 256, 4)
    old = E.CONV_MODE
    E.CONV_MODE = "f32"
    try:
        TM.test_model_matches_reference(goldens, name, "f32")
    finally:
        E.CONV_MODE = old


def test_train_step_at_d_model_128():
    """One fused train step of TimeUNet at d_model = 128 (head width 8): the L-TAE runs the 16-pixel / 8-pixel family at the
    full 16 x 16 resolution; finite loss, every trainable parameter moved."""
    import crop2seg_amd as C2S
    import test_models_gpu as TM
    from crop2seg_amd.learning.utils import TrainStep
    from oracle import seeded
    net = C2S.TimeUNet_v1(input_dim=10, out_conv=[32, 15], d_model=128)
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 43, "tame"))
    net = net.cuda().train()
    net.spec.attn_dropout = 0.0
    net.spec.mlp_dropout = 0.0
    x, dates, y = seeded.make_inputs(1, 4, 10, 16, 16, 312, None)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    step = TrainStep(net, num_classes=15)
    loss, logits = step(x.cuda(), dates.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(logits).all())
    after = dict(net.named_parameters())
    # (biases in front of a batch-statistics norm and fc1_k.bias have a gradient that is 0 up to rounding -- the names
    # test_models_gpu._abs_only lists: an exact 0 there leaves the parameter where it was)
    same = [n for n, p in before.items() if after[n].requires_grad and torch.equal(p, after[n].detach())
            and not TM._abs_only(n, True)]
    assert not same, same
    assert any(not torch.equal(p, after[n].detach()) for n, p in before.items() if n.startswith("temporal_encoder.attention_head"))
    assert step.ws.sync_error() == 0
