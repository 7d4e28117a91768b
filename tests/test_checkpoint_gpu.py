"""Snapshots, checkpoints and resume on the GPU (csrc/snapshot.hip, crop2seg_amd/checkpoint.py, TrainStep.snapshot / load).

Kernel level: gather, verify and scatter between poisoned guard bands against the numpy restatement (snapshot_ref).  Above:
a resumed run equals the uninterrupted one bit for bit -- eager, with a freeze schedule, guarded with a skipped step, and
replayed from a captured graph.  Every bit-exact case first asserts that two uninterrupted runs agree, so that a difference
there is not blamed on resume; the eager case also shows that the seed record is what makes the resumed run agree."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import snapshot_ref as R  # noqa: E402
from redzone import POISON_I32, arena  # noqa: E402

MODELS = ("utae", "wtae", "timeunet")
ENCODER = {"utae": ("in_conv.", "down_blocks."), "wtae": ("in_conv.", "down_blocks.", "spatial_reduction."),
           "timeunet": ("in_conv.",)}
SEED_A, SEED_B = 0, 1234          # torch.manual_seed of the original and of the resuming process


# ================================================================================================== kernel level
SPAN = R.SPAN_BYTES
# (bytes, element size, misalignment of the address in bytes)
REGIONS = [(0, 4, 0), (4, 4, 4), (8, 8, 8), (12, 4, 12), (16, 4, 0), (20, 4, 8), (16, 8, 8), (SPAN - 4, 4, 0), (SPAN, 4, 4),
           (SPAN + 4, 4, 12), (SPAN + 8, 8, 0), (SPAN * R.MAX_BLOCKS + 20, 4, 4), (24, 8, 0), (0, 8, 8), (40, 4, 0)]
SLACK = 4                         # words around a region inside its own block


def _backing(nbytes, elem, mis, fill):
    """A block of the arena holding SLACK words, the region at `mis` bytes past a 16-byte boundary, and SLACK words; returns
    (block as int32, region as a tensor of its element type)."""
    words = nbytes // 4
    lead = SLACK + mis // 4
    block = torch.empty(lead + words + SLACK, dtype=torch.int32, device="cuda")     # 512-byte aligned, poisoned
    if fill is not None:
        block[lead:lead + words] = fill
    region = block[lead:lead + words]
    assert words == 0 or region.data_ptr() % 16 == mis
    return block, (region.view(torch.int64) if elem == 8 else region)


def _table(E, regions, offs):
    return E.snapshot_table([r.data_ptr() for r in regions], [r.numel() * r.element_size() for r in regions], offs, "cuda")


def _slack_intact(block, words):
    lead = block.numel() - words - SLACK
    return bool((block[:lead] == POISON_I32).all()) and bool((block[lead + words:] == POISON_I32).all())


def test_gather_verify_scatter_between_guard_bands():
    from crop2seg_amd import checkpoint as CK
    from crop2seg_amd import engine as E
    rng = np.random.default_rng(11)
    data = [torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, nb // 4, dtype=np.int64).astype(np.int32)) for nb, _, _ in REGIONS]
    sizes = [nb for nb, _, _ in REGIONS]
    offs, payload, _ = CK.plan_layout(sizes)
    assert max(sizes) > R.MAX_BLOCKS * SPAN, "one region larger than the grid's first pass"
    want = R.blob([d.numpy() for d in data])
    with arena("cuda", 160 << 20) as a:
        src = [_backing(nb, el, mis, d.cuda()) for (nb, el, mis), d in zip(REGIONS, data)]
        table = _table(E, [r for _, r in src], offs)
        blob = torch.empty(R.HEADER_BYTES + payload, dtype=torch.uint8, device="cuda")          # poisoned: every byte is written
        E.snapshot_gather(table, len(REGIONS), blob)
        torch.cuda.synchronize()
        got = blob.cpu().numpy()
        assert got[:64].tobytes() == want[:64].tobytes(), (CK.parse_header(got[:64].tobytes()), CK.parse_header(want[:64].tobytes()))
        assert np.array_equal(got, want), "blob differs from the restatement"
        for (b, _), (nb, _, _) in zip(src, REGIONS):
            assert _slack_intact(b, nb // 4), "gather wrote around a live region"

        # scatter into poisoned destinations
        status = E.snapshot_status("cuda")
        dst = [_backing(nb, el, mis, None) for nb, el, mis in REGIONS]
        dtable = _table(E, [r for _, r in dst], offs)
        E.snapshot_verify(blob, len(REGIONS), status)
        E.snapshot_scatter(dtable, len(REGIONS), blob, status)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        assert st.view(np.int32)[:2].tolist() == [1, 0]
        assert (int(st.view(np.uint64)[1]), int(st.view(np.uint64)[2])) == R.sums(want[64:].view(np.uint32))
        for (b, r), (_, s), (nb, _, _) in zip(dst, src, REGIONS):
            assert torch.equal(r, s), f"region of {nb} bytes"
            assert _slack_intact(b, nb // 4), f"scatter wrote around the region of {nb} bytes"

        # refused blobs leave every destination byte alone
        dst2 = [_backing(nb, el, mis, None) for nb, el, mis in REGIONS]
        dtable2 = _table(E, [r for _, r in dst2], offs)
        big = offs[sizes.index(max(sizes))]
        cases = {"payload bit": (R.HEADER_BYTES + big + 4 * 1000003 + 2, 0x10, 5), "region count": (8, 0x01, 3), "magic": (1, 0x40, 1),
                 "padding bit": (R.HEADER_BYTES + offs[1] + 4, 0x01, 5)}
        for what, (byte, bit, reason) in cases.items():
            bad = blob.clone()
            bad[byte] ^= bit
            assert R.check(bad.cpu().numpy(), len(REGIONS)) == reason
            E.snapshot_verify(bad, len(REGIONS), status)
            E.snapshot_scatter(dtable2, len(REGIONS), bad, status)
            torch.cuda.synchronize()
            assert status.cpu().numpy().view(np.int32)[:2].tolist() == [0, reason], what
            for b, _ in dst2:
                assert bool((b == POISON_I32).all()), f"{what}: a refused blob reached a destination"
        # a sound blob offered with another region count is refused as well
        E.snapshot_verify(blob, len(REGIONS) - 1, status)
        E.snapshot_scatter(dtable2, len(REGIONS) - 1, blob, status)
        torch.cuda.synchronize()
        assert status.cpu().numpy().view(np.int32)[:2].tolist() == [0, 3]
        assert all(bool((b == POISON_I32).all()) for b, _ in dst2)


def test_gather_inside_a_captured_graph():
    from crop2seg_amd import checkpoint as CK
    from crop2seg_amd import engine as E
    sizes = [4, SPAN + 12, 0, 40, 3 * SPAN]
    offs, payload, _ = CK.plan_layout(sizes)
    g = torch.Generator("cuda").manual_seed(3)
    live = [torch.randint(-(1 << 31), 1 << 31, (n // 4,), device="cuda", generator=g).to(torch.int32) for n in sizes]
    table = _table(E, live, offs)
    blob_g = torch.zeros(R.HEADER_BYTES + payload, dtype=torch.uint8, device="cuda")
    blob_e = torch.zeros_like(blob_g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        E.snapshot_gather(table, len(sizes), blob_g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E.snapshot_gather(table, len(sizes), blob_g)
    for k in range(2):
        for t in live:
            t.add_(k + 1)                            # the graph reads the live regions anew at every replay
        graph.replay()
        E.snapshot_gather(table, len(sizes), blob_e)
        torch.cuda.synchronize()
        assert torch.equal(blob_g, blob_e)
        assert np.array_equal(blob_g.cpu().numpy(), R.blob([t.cpu().numpy() for t in live]))


# ================================================================================================== TrainStep
def _net(model, seed=SEED_A, **kw):
    """The models of tests/test_frozen_gpu.py (seeded "tame" weights), dropout left at the models' defaults; `seed` is the
    process's torch.manual_seed, the root of the dropout sequence."""
    import crop2seg_amd as C2S
    from oracle import seeded
    torch.manual_seed(seed)
    cls = {"utae": C2S.UTAE, "wtae": C2S.WTAE, "timeunet": C2S.TimeUNet_v1}[model]
    net = cls(input_dim=10, out_conv=[32, 15], **kw)
    ks = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict(seeded.make_state(ks, 3, "tame"))
    return net.cuda().train()


_INPUTS = {}


def _inputs():
    if not _INPUTS:
        from oracle import seeded
        x, dates, y = seeded.make_inputs(2, 5, 10, 32, 32, 91, [5, 3])
        xn = x.clone()
        xn[1, 2, 3, 17, 5] = float("nan")
        _INPUTS.update(x=x.cuda(), dates=dates.cuda(), y=y.cuda(), xn=xn.cuda())
    return _INPUTS["x"], _INPUTS["dates"], _INPUTS["y"]


def _step(net, **kw):
    from crop2seg_amd.learning.utils import TrainStep
    return TrainStep(net, num_classes=15, **kw)


def _state(step, loss=None):
    torch.cuda.synchronize()
    out = {"flat_param": step.flat_param.clone(), "exp_avg": step.exp_avg.clone(), "exp_avg_sq": step.exp_avg_sq.clone(),
           "param_steps": list(step.param_steps)}
    out.update({"buffer:" + k: b.clone() for k, b in step.model.named_buffers()})
    if loss is not None:
        out["loss"] = loss.clone()
    return out


def _diff(a, b):
    """Names of the entries that differ (bitwise for tensors; NaN equals NaN bit for bit)."""
    assert sorted(a) == sorted(b)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    return [k for k in a if (not torch.equal(bits(a[k]), bits(b[k])) if torch.is_tensor(a[k]) else a[k] != b[k])]


def _freeze(net, model, flag):
    for n, p in net.named_parameters():
        if n.startswith(ENCODER[model]):
            p.requires_grad_(flag)


def _run(model, nsteps, seed=SEED_A, **kw):
    x, dates, y = _inputs()
    step = _step(_net(model, seed), **kw)
    loss = None
    for _ in range(nsteps):
        loss, _ = step(x, dates, y)
    return step, loss


@pytest.mark.parametrize("model", MODELS)
def test_eager_resume_is_bit_exact_and_needs_the_seed_record(model, tmp_path):
    from crop2seg_amd import checkpoint as CK
    x, dates, y = _inputs()
    step_a, loss_a = _run(model, 4)
    want = _state(step_a, loss_a)
    step_t, loss_t = _run(model, 4)
    assert _diff(want, _state(step_t, loss_t)) == [], "two uninterrupted runs differ: not a matter of resume"
    step_b, _ = _run(model, 2)
    path = str(tmp_path / "model.pth.tar")
    step_b.snapshot().save(path, epoch=7, best_mIoU=0.25)

    step_c = _step(_net(model, SEED_B))
    info = step_c.load(path)
    assert info == {"bit_exact": True, "epoch": 7, "best_mIoU": 0.25}
    assert all(p.data_ptr() == step_c.flat_param.data_ptr() + 4 * o for (_, p), o in zip(step_c._named, step_c.offsets))
    for _ in range(2):
        loss_c, _ = step_c(x, dates, y)
    assert _diff(want, _state(step_c, loss_c)) == []
    assert step_c.step_count == 4

    # the control: the same state without the seed record, under the resuming process's own seed
    state = torch.load(path, map_location="cpu", weights_only=True)
    del state[CK.EXTRA_KEY]
    step_d = _step(_net(model, SEED_B))
    with pytest.warns(UserWarning, match="not bit-exact"):
        assert step_d.load_state_dict(state)["bit_exact"] is False
    assert _diff(_state(step_b), _state(step_d)) == [], "a reference-format state loads parameters, buffers, moments, counts"
    for _ in range(2):
        step_d(x, dates, y)
    assert "flat_param" in _diff({k: v for k, v in want.items() if k != "loss"}, _state(step_d)), "dropout is off or unseeded: this resume test would prove nothing"


def test_snapshot_is_ordered_with_the_stream():
    x, dates, y = _inputs()
    step, _ = _run("utae", 1)
    torch.cuda.synchronize()
    at = _state(step)
    snap = step.snapshot()
    for _ in range(2):                               # launched at once, while the copy is under way
        step(x, dates, y)
    snap.wait()
    for k in ("flat_param", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(snap.region(k).view(np.int32), at[k].cpu().numpy().view(np.int32)), k
    assert _diff({k: at[k] for k in ("flat_param",)}, {"flat_param": step.flat_param}) == ["flat_param"]     # the state has moved on
    sd = snap.state_dict()["state_dict"]
    assert list(sd) == list(step.model.state_dict())
    # three in a row, a step between them: two staging blobs, the third waits for the first
    snaps, clones = [], []
    for _ in range(3):
        snaps.append(step.snapshot())
        clones.append((step.flat_param.clone(), step.exp_avg_sq.clone()))        # stream-ordered with the snapshot
        step(x, dates, y)
    for s, (p, v) in zip(snaps, clones):
        assert np.array_equal(s.region("flat_param").view(np.int32), p.cpu().numpy().view(np.int32))
        assert np.array_equal(s.region("exp_avg_sq").view(np.int32), v.cpu().numpy().view(np.int32))
        s.state_dict()                               # header against payload
    assert not np.array_equal(snaps[0].region("flat_param"), snaps[2].region("flat_param"))


def test_frozen_schedule_resumes_bit_exact_with_torch_step_counts(tmp_path):
    model = "utae"
    x, dates, y = _inputs()

    def schedule(step, first, ref=None, opt=None):
        loss = None
        for k in range(first, 6):
            _freeze(step.model, model, not (2 <= k < 4))
            loss, _ = step(x, dates, y)
            if opt is not None:
                for (n, p), r in zip(step.model.named_parameters(), ref):
                    r.grad = step.grads[n].clone() if p.requires_grad else None
                opt.step()
        return loss

    runs = []
    for _ in range(2):
        step = _step(_net(model))
        runs.append(_state(step, schedule(step, 0)))
    assert _diff(*runs) == [], "two uninterrupted runs differ: not a matter of resume"
    step_b, _ = _run(model, 2)
    path = str(tmp_path / "ckpt.pth.tar")
    step_b.snapshot().save(path)
    step_c = _step(_net(model, SEED_B))
    step_c.load(path)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    ref = [p.detach().clone().requires_grad_(True) for p in step_c.model.parameters()]
    opt = torch.optim.Adam(ref, lr=1e-3)
    opt.load_state_dict(ckpt["optimizer"])
    loss_c = schedule(step_c, 2, ref, opt)
    assert _diff(runs[0], _state(step_c, loss_c)) == []
    for n, r in zip(step_c.names, ref):
        assert int(opt.state[r]["step"]) == step_c.param_steps[step_c.names.index(n)], n
    assert sorted(set(step_c.param_steps)) == [4, 6]


def test_guarded_resume_after_a_skipped_step(tmp_path):
    x, dates, y = _inputs()
    xn = _INPUTS["xn"]
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True)

    def run(n_clean, seed=SEED_A):
        step = _step(_net("utae", seed, encoder_norm="batch"), **kw)
        loss, _ = step(xn, dates, y)                 # skipped on the device
        for _ in range(n_clean):
            loss, _ = step(x, dates, y)
        return step, loss

    step_a, loss_a = run(2)
    want = _state(step_a, loss_a)
    kinds = {b.dtype for b in step_a.model.buffers()}
    assert torch.float32 in kinds and torch.int64 in kinds, "the model must have float and int64 buffers"
    step_t, loss_t = run(2)
    assert _diff(want, _state(step_t, loss_t)) == [], "two uninterrupted runs differ: not a matter of resume"
    step_b, _ = run(0)
    path = str(tmp_path / "guarded.pth.tar")
    step_b.snapshot().save(path)
    step_c = _step(_net("utae", SEED_B, encoder_norm="batch"), **kw)
    step_c.load(path)
    assert all(b.data_ptr() >= step_c.flat_buf.data_ptr() for b in step_c.model.buffers() if b.is_floating_point())
    assert step_c.skipped_steps() == 1 and step_c.step_count == 0 and set(step_c.param_steps) == {0}
    for _ in range(2):
        loss_c, _ = step_c(x, dates, y)
    got = _state(step_c, loss_c)
    got["param_steps"] = want["param_steps"] = None      # the hosts' counts are compared after sync_steps() below
    assert _diff(want, got) == []
    assert step_c.skipped_steps() == step_a.skipped_steps() == 1
    step_a.sync_steps()
    step_c.sync_steps()
    assert step_c.param_steps == step_a.param_steps and set(step_c.param_steps) == {2}
    assert step_c.step_count == step_a.step_count == 2
    # a guarded state does not go into an unguarded step
    plain = _step(_net("utae", SEED_B, encoder_norm="batch"))
    before = _state(plain)
    with pytest.raises(ValueError, match="guard mode"):
        plain.load(path)
    assert _diff(before, _state(plain)) == []


def test_replayed_resume_and_roll_back(tmp_path):
    from crop2seg_amd import checkpoint as CK
    x, dates, y = _inputs()

    def run(n, seed=SEED_A):
        step = _step(_net("utae", seed))
        step.capture(x, dates, y)
        loss = None
        for _ in range(n):
            loss, _ = step.replay()
        return step, loss

    step_a, loss_a = run(4)
    want = _state(step_a, loss_a)
    step_t, loss_t = run(4)
    assert _diff(want, _state(step_t, loss_t)) == [], "two uninterrupted runs differ: not a matter of resume"
    step_b, _ = run(2)
    path = str(tmp_path / "replay.pth.tar")
    step_b.snapshot().save(path)

    step_c = _step(_net("utae", SEED_B))
    step_c.load(path)
    step_c.capture(x, dates, y)
    for _ in range(2):
        loss_c, _ = step_c.replay()
    assert _diff(want, _state(step_c, loss_c)) == []

    # roll the captured original back to its own snapshot: the graphs stay, the continuation is the same
    step_b.replay()
    graphs = (step_b.graph_fb, step_b.graph_opt)
    step_b.load(path)
    assert (step_b.graph_fb, step_b.graph_opt) == graphs and graphs[0] is not None
    for _ in range(2):
        loss_b, _ = step_b.replay()
    assert _diff(want, _state(step_b, loss_b)) == []

    # another dropout base does not fit the baked one
    state = torch.load(path, map_location="cpu", weights_only=True)
    state[CK.EXTRA_KEY]["seed_root"] += 1
    before = _state(step_b)
    with pytest.raises(RuntimeError, match="capture"):
        step_b.load_state_dict(state)
    eager = dict(state)
    eager[CK.EXTRA_KEY] = dict(state[CK.EXTRA_KEY], capture=None)
    with pytest.raises(RuntimeError, match="capture"):
        step_b.load_state_dict(eager)
    assert _diff(before, _state(step_b)) == []


def test_damaged_and_foreign_states_are_refused_untouched(tmp_path):
    x, dates, y = _inputs()
    step = _step(_net("utae", encoder_norm="batch"))
    for _ in range(2):
        step(x, dates, y)
    path = str(tmp_path / "good.pth.tar")
    step.snapshot().save(path)
    step(x, dates, y)
    before = _state(step)
    name = step.names[5]
    for where in ("state_dict", "exp_avg"):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        t = ckpt["state_dict"][name] if where == "state_dict" else ckpt["optimizer"]["state"][5]["exp_avg"]
        t.view(torch.int32).reshape(-1)[0] ^= 1 << 3                           # one flipped bit
        bad = str(tmp_path / f"bad_{where}.pth.tar")
        torch.save(ckpt, bad)
        with pytest.raises(RuntimeError, match="refused"):
            step.load(bad)
        assert _diff(before, _state(step)) == [], where
    other = _step(_net("wtae", SEED_B))
    foreign = other.snapshot().state_dict()
    with pytest.raises(ValueError, match="does not fit"):
        step.load_state_dict(foreign)
    assert _diff(before, _state(step)) == []
    step.load(path)                                                            # the sound file still loads
    assert step.step_count == 2 and _diff(before, _state(step)) != []


def test_file_loads_into_torch_adam_and_a_second_model():
    """After 3 steps the file's optimiser state goes into torch.optim.Adam over CPU clones of the parameters; torch's step 4 on
    TrainStep's step-4 gradient equals TrainStep's own step 4 within 1e-6 relative per parameter."""
    from crop2seg_amd.backbones.functional import DropoutState
    x, dates, y = _inputs()
    step, _ = _run("utae", 3)
    ckpt = step.snapshot().state_dict()
    net2 = _net("utae", SEED_B)
    net2.load_state_dict(ckpt["state_dict"], strict=True)
    assert list(ckpt["state_dict"]) == list(step.model.state_dict())
    for (k, a), (_, b) in zip(step.model.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a, b), k
    ref = [ckpt["state_dict"][n].clone().requires_grad_(True) for n in step.names]
    opt = torch.optim.Adam(ref, lr=1e-3)
    opt.load_state_dict(ckpt["optimizer"])
    assert all(float(s["step"]) == 3.0 and s["step"].dtype == torch.float32 for s in ckpt["optimizer"]["state"].values())
    drop = DropoutState(attn_seed=5, mlp_seed=6)
    step(x, dates, y, dropout_state=drop, apply_update=False)
    for n, r in zip(step.names, ref):
        r.grad = step.grads[n].detach().cpu().clone()
    opt.step()
    step(x, dates, y, dropout_state=drop)
    torch.cuda.synchronize()
    for n, r in zip(step.names, ref):
        got = step.params[n].detach().cpu().double()
        err = float((got - r.detach().double()).norm() / (r.detach().double().norm() + 1e-30))
        assert err < 1e-6, (n, err)
