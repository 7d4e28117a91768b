"""Fine-tuning with frozen parameters (requires_grad False) on the GPU: the pruned backward gives the trainable parameters the
gradients of the all-trainable backward bit for bit, on the drop-in and the TrainStep paths; frozen parameters get no
launch of their own and no update; the kernels' input-gradient-free modes give bit-identical parameter outputs."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = ("utae", "wtae", "timeunet")
ENCODER = {"utae": ("in_conv.", "down_blocks."), "wtae": ("in_conv.", "down_blocks.", "spatial_reduction."),
           "timeunet": ("in_conv.",)}
PATTERNS = ("encoder", "encoder+te", "te", "norm_weight")
# the frozen blocks in front of the temporal encoder (W-TAE's down_blocks run after the aggregation: their input trains)
UPSTREAM = {"utae": ("in_conv.", "down_blocks."), "wtae": ("in_conv.", "spatial_reduction."), "timeunet": ("in_conv.",)}


def _frozen_prefixes(model, pattern):
    if pattern == "encoder":
        return ENCODER[model]
    if pattern == "encoder+te":
        return ENCODER[model] + ("temporal_encoder.",)
    if pattern == "te":
        return ("temporal_encoder.",)
    return ("in_conv.conv.conv.1.weight",)              # one GroupNorm's gamma (its beta trains)


def _net(model):
    import crop2seg_amd as C2S
    from oracle import seeded
    torch.manual_seed(0)
    cls = {"utae": C2S.UTAE, "wtae": C2S.WTAE, "timeunet": C2S.TimeUNet_v1}[model]
    net = cls(input_dim=10, out_conv=[32, 15])
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    net = net.cuda().train()
    net.spec.attn_dropout = 0.0
    net.spec.mlp_dropout = 0.0
    return net


def _inputs():
    from oracle import seeded
    x, dates, y = seeded.make_inputs(2, 5, 10, 32, 32, 91, [5, 3])      # padded frames in the second series
    return x.cuda(), dates.cuda(), y.cuda()


def _freeze(net, prefixes, flag=False):
    frozen = []
    for n, p in net.named_parameters():
        if n.startswith(prefixes):
            p.requires_grad_(flag)
            frozen.append(n)
    assert frozen
    return frozen


def _dropin_grads(net, x, dates, gout):
    for p in net.parameters():
        p.grad = None
    out = net(x, batch_positions=dates)
    out.backward(gout)
    torch.cuda.synchronize()
    return {n: (p.grad.clone() if p.grad is not None else None) for n, p in net.named_parameters()}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_dropin_gradients_equal_the_all_trainable_backward(model, pattern):
    net = _net(model)
    x, dates, _ = _inputs()
    gout = torch.randn(2, 15, 32, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    ref = _dropin_grads(net, x, dates, gout)
    frozen = set(_freeze(net, _frozen_prefixes(model, pattern)))
    got = _dropin_grads(net, x, dates, gout)
    for n, g in got.items():
        if n in frozen:
            assert g is None, n
        else:
            assert torch.equal(g, ref[n]), n


def _step(net):
    from crop2seg_amd.learning.utils import TrainStep
    return TrainStep(net, num_classes=15)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_trainstep_gradients_and_launch_log(model, pattern):
    from crop2seg_amd import engine as E
    from crop2seg_amd.backbones.functional import DropoutState
    net = _net(model)
    x, dates, y = _inputs()
    step = _step(net)
    step(x, dates, y, dropout_state=DropoutState(), apply_update=False)
    ref = {n: g.clone() for n, g in step.grads.items()}
    prefixes = _frozen_prefixes(model, pattern)
    frozen = set(_freeze(net, prefixes))
    step.flat_grad.fill_(7.0)                           # frozen slots must keep this
    E.BACKWARD_LOG = []
    try:
        step(x, dates, y, dropout_state=DropoutState(), apply_update=False)
        torch.cuda.synchronize()
        log = list(E.BACKWARD_LOG)
    finally:
        E.BACKWARD_LOG = None
    for n, g in step.grads.items():
        if n in frozen:
            assert bool((g == 7.0).all()), f"frozen slot {n} was written"
        else:
            assert torch.equal(g, ref[n]), n
    assert log, "no backward launch logged"
    assert not [e for e in log if e[2] == "wgrad" and e[1] in frozen], "weight gradient of a frozen weight"
    if pattern.startswith("encoder"):
        # the per-frame encoder's tensors and the temporal encoder's input have only frozen parameters upstream
        up = UPSTREAM[model]
        assert not [e for e in log if e[2] == "dgrad" and (e[1].startswith(up) or e[0] in ("ltae", "temporal_aggregate"))], log
    if pattern == "encoder+te":
        assert not [e for e in log if e[0] == "ltae"]


@pytest.mark.parametrize("model", MODELS)
def test_trainstep_leaves_frozen_parameters_and_moments_untouched(model):
    from crop2seg_amd.backbones.functional import DropoutState
    x, dates, y = _inputs()
    net_a = _net(model)
    step_a = _step(net_a)
    step_a(x, dates, y, dropout_state=DropoutState())
    net_f = _net(model)
    step_f = _step(net_f)
    frozen = set(_freeze(net_f, ENCODER[model]))
    before = {n: (step_f.params[n].clone(), step_f.exp_avg[o:o + p.numel()].clone(), step_f.exp_avg_sq[o:o + p.numel()].clone())
              for (n, p), o in zip(net_f.named_parameters(), step_f.offsets) if n in frozen}
    step_f(x, dates, y, dropout_state=DropoutState())
    torch.cuda.synchronize()
    # BatchNorm running statistics follow the same first forward (torch updates them for frozen layers too)
    for (k, a), (_, f) in zip(net_a.named_buffers(), net_f.named_buffers()):
        assert torch.equal(a, f), k
    for _ in range(2):
        step_f(x, dates, y, dropout_state=DropoutState())
    torch.cuda.synchronize()
    for (n, p), o in zip(net_f.named_parameters(), step_f.offsets):
        if n in frozen:
            p0, m0, v0 = before[n]
            assert torch.equal(step_f.params[n], p0), n
            assert torch.equal(step_f.exp_avg[o:o + p.numel()], m0), n
            assert torch.equal(step_f.exp_avg_sq[o:o + p.numel()], v0), n
    assert step_f.param_steps == [0 if n in frozen else 3 for n in step_f.names]


@pytest.mark.parametrize("model", MODELS)
def test_freeze_unfreeze_schedule_matches_torch_adam(model):
    """2 steps all trainable, 2 with the encoder frozen, 2 unfrozen: TrainStep's parameters against torch.optim.Adam fed the
    same gradients (None for a frozen parameter, as autograd leaves it): a frozen parameter's step count, and so its bias
    correction, does not advance."""
    from crop2seg_amd.backbones.functional import DropoutState
    x, dates, y = _inputs()
    net = _net(model)
    step = _step(net)
    ref = [p.detach().clone().requires_grad_(True) for p in net.parameters()]
    opt = torch.optim.Adam(ref, lr=1e-3)
    for k in range(6):
        flag = not (2 <= k < 4)
        for n, p in net.named_parameters():
            if n.startswith(ENCODER[model]):
                p.requires_grad_(flag)
        step(x, dates, y, dropout_state=DropoutState())
        for (n, p), r in zip(net.named_parameters(), ref):
            r.grad = step.grads[n].clone() if p.requires_grad else None
        opt.step()
    torch.cuda.synchronize()
    for (n, p), r in zip(net.named_parameters(), ref):
        err = float((p.detach() - r.detach()).norm() / (r.detach().norm() + 1e-30))
        assert err < 1e-6, (n, err)
        assert int(opt.state[r]["step"]) == step.param_steps[step.names.index(n)], n


def test_hipgraph_with_a_frozen_encoder_replays_eager_steps():
    from crop2seg_amd.backbones.functional import DropoutState
    x, dates, y = _inputs()
    net_e = _net("utae")
    step_e = _step(net_e)
    _freeze(net_e, ENCODER["utae"])
    for _ in range(3):
        loss_e, _ = step_e(x, dates, y, dropout_state=DropoutState())
    net_g = _net("utae")
    step_g = _step(net_g)
    _freeze(net_g, ENCODER["utae"])
    step_g.capture(x, dates, y)
    for _ in range(3):
        loss_g, _ = step_g.replay()
    torch.cuda.synchronize()
    assert float(loss_g) == float(loss_e)
    assert torch.equal(step_g.flat_param, step_e.flat_param)
    assert torch.equal(step_g.exp_avg, step_e.exp_avg) and torch.equal(step_g.exp_avg_sq, step_e.exp_avg_sq)
    next(net_g.in_conv.parameters()).requires_grad_(True)
    with pytest.raises(RuntimeError, match="capture"):
        step_g.replay()


# ----------------------------------------------------------------------------------------------------------------- kernel modes
def test_temporal_aggregate_without_input_gradient():
    from crop2seg_amd import _lib
    L = _lib.lib()
    g = torch.Generator("cuda").manual_seed(3)
    B, T, Cc, H, W, nh, h, w = 2, 5, 64, 32, 32, 16, 8, 8
    x = torch.randn(B, T, Cc, H, W, device="cuda", generator=g)
    attn = torch.rand(nh, B, T, h, w, device="cuda", generator=g)
    gout = torch.randn(B, Cc, H, W, device="cuda", generator=g)
    valid = torch.tensor([1] * 5 + [1, 1, 1, 0, 0], device="cuda", dtype=torch.int32)
    d = _lib.AggDesc(B, T, Cc, H, W, nh, h, w)
    ws = torch.empty(L.c2s_temporal_aggregate_bwd_workspace_floats(C.byref(d)), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    gx = torch.empty_like(x)
    ga_full, ga = torch.zeros_like(attn), torch.zeros_like(attn)
    assert L.c2s_temporal_aggregate_bwd(C.byref(d), x.data_ptr(), attn.data_ptr(), valid.data_ptr(), gout.data_ptr(),
                                        gx.data_ptr(), 0, ga_full.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    assert L.c2s_temporal_aggregate_bwd(C.byref(d), x.data_ptr(), attn.data_ptr(), valid.data_ptr(), gout.data_ptr(),
                                        None, 0, ga.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(ga, ga_full)


@pytest.mark.parametrize("onepass", [False, True])
@pytest.mark.parametrize("kind,N,Cc,HW,groups,valid", [
    ("group", 6, 64, 64 * 64, 4, True), ("batch", 4, 32, 32 * 32, 1, False), ("group", 3, 128, 16 * 16, 4, False)])
def test_norm_backward_without_input_gradient(onepass, kind, N, Cc, HW, groups, valid):
    from crop2seg_amd import _lib
    L = _lib.lib()
    g = torch.Generator("cuda").manual_seed(4)
    k = _lib.NORM_BATCH if kind == "batch" else _lib.NORM_GROUP
    d = _lib.NormDesc(N, Cc, HW, k, groups, 1, 1e-5, 0.1)
    x = torch.randn(N, Cc, HW, device="cuda", generator=g)
    gy = torch.randn(N, Cc, HW, device="cuda", generator=g)
    gamma, beta = torch.randn(Cc, device="cuda", generator=g), torch.randn(Cc, device="cuda", generator=g)
    vf = torch.tensor([1] * (N - 1) + [0], device="cuda", dtype=torch.int32) if valid else None
    vp = vf.data_ptr() if valid else None
    ng = Cc if kind == "batch" else N * groups
    gstats, row_ab = torch.empty(2 * ng, device="cuda"), torch.empty(3 * N * Cc, device="cuda")
    ws = torch.empty(L.c2s_norm_workspace_floats(C.byref(d)), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    y = torch.empty_like(x)
    rm, rv = torch.zeros(Cc, device="cuda"), torch.ones(Cc, device="cuda")
    sync_b = L.c2s_norm_onepass_sync_bytes(C.byref(d), 1 if valid else 0) if onepass else 0
    if onepass and sync_b == 0:
        pytest.skip("shape not taken by the one-pass form")
    sync = torch.zeros(max(sync_b, 4096), device="cuda", dtype=torch.uint8)
    assert L.c2s_norm_fwd(C.byref(d), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), None,
                          gstats.data_ptr(), row_ab.data_ptr(), None, y.data_ptr(), 1, ws.data_ptr(), ws.numel(), vp, 0.0, st) == 0
    outs = []
    for with_gx in (True, False):
        gx = torch.empty_like(x) if with_gx else None
        dg, db = torch.empty(Cc, device="cuda"), torch.empty(Cc, device="cuda")
        args = (C.byref(d), x.data_ptr(), gy.data_ptr(), gamma.data_ptr(), gstats.data_ptr(), row_ab.data_ptr(), 1,
                None if gx is None else gx.data_ptr(), dg.data_ptr(), db.data_ptr(), None, ws.data_ptr(), ws.numel(), vp)
        if onepass:
            rc = L.c2s_norm_bwd_onepass(*args, sync.data_ptr(), sync.numel(), st)
        else:
            rc = L.c2s_norm_bwd(*args, st)
        assert rc == 0
        outs.append((dg, db))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# B, T, C, h, with_emb, pad, drop, need_attn ; environment -> the backward path it must take
LTAE_PATH_RUNS = [
    ({"C2S_LTAE_LDS": "0", "C2S_LTAE_LDS_BWD": "0"}, ["2,6,128,4,1,1,0,1,0", "2,7,128,4,0,1,1,1,0"]),
    ({"C2S_LTAE_REG": "0", "C2S_LTAE_REG_BWD": "0", "C2S_LTAE_GX64": "0"}, ["2,5,64,128,1,1,1,1,1"]),
    ({"C2S_LTAE_REG_BWD": "0"}, ["2,5,64,128,1,1,1,1,2"]),
    ({}, ["2,5,64,128,1,1,1,1,3", "2,5,64,128,1,1,1,0,4", "2,6,128,4,1,1,0,1,5", "1,9,256,8,1,1,1,1,5",
          "1,70,64,16,1,1,1,1,6"]),
]


@pytest.mark.parametrize("env,cases", LTAE_PATH_RUNS)
def test_ltae_backward_without_input_gradient_on_every_path(env, cases):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ltae_nogx_worker.py"), *cases],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"LTAE_NOGX_OK {len(cases)}" in r.stdout, r.stdout[-3000:]
