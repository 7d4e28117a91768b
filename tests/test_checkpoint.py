"""Checkpoints without a GPU: the blob layout planner against the numpy restatement, what the two checksums detect, the
conversion between the flat training state and torch's file format, and the ABI of the new entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import snapshot_ref as R  # noqa: E402

MIXED_300 = [(4 if i % 3 else 8) * ((i * 7) % 23) for i in range(300)]      # 4- and 8-byte elements, some regions empty
BYTE_LISTS = [[4], [0, 4], [12, 20, 16], MIXED_300]


@pytest.mark.parametrize("sizes", BYTE_LISTS, ids=["4", "0-4", "12-20-16", "mixed300"])
def test_layout_planner_matches_the_restatement(sizes):
    from crop2seg_amd import checkpoint as CK
    offs, payload, blocks = CK.plan_layout(sizes)
    assert (offs, payload) == R.layout(sizes)
    assert blocks == R.block_starts(sizes)
    assert all(o % 16 == 0 for o in offs) and payload % 16 == 0
    assert all(offs[i] + sizes[i] <= (offs[i + 1] if i + 1 < len(offs) else payload) for i in range(len(sizes)))
    # the header and the sums of a blob built from these regions
    rng = np.random.default_rng(len(sizes))
    regions = [rng.integers(0, 1 << 32, n // 4, dtype=np.uint32) for n in sizes]
    blob = R.blob(regions)
    h = CK.parse_header(blob[:64].tobytes())
    parts = [(o,) + CK.word_sums(r) for o, r in zip(offs, regions)]
    assert h == {"magic": R.MAGIC, "version": R.VERSION, "nregions": len(sizes), "payload_bytes": payload,
                 "s1": CK.compose_sums(parts)[0], "s2": CK.compose_sums(parts)[1]}
    assert CK.blob_header(len(sizes), payload, h["s1"], h["s2"]) == blob[:64].tobytes()
    assert CK.word_sums(blob[64:]) == (h["s1"], h["s2"])
    assert not blob[40:64].any()
    for o, n in zip(offs, sizes):                                              # padding words are 0
        assert not blob[64 + o + n:64 + o + -(-n // 16) * 16].any()


def test_plan_layout_refuses_odd_sizes():
    from crop2seg_amd import checkpoint as CK
    for bad in ([6], [-4], [4, 3]):
        with pytest.raises(ValueError):
            CK.plan_layout(bad)


def test_constants_agree_with_the_header():
    from crop2seg_amd import engine as E
    src = open(os.path.join(ROOT, "include", "c2s_hip.h")).read()
    macro = lambda n: int(re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % n, src).group(1), 0)
    assert macro("C2S_SNAPSHOT_HEADER_BYTES") == E.SNAPSHOT_HEADER_BYTES == R.HEADER_BYTES
    assert macro("C2S_SNAPSHOT_SPAN_BYTES") == E.SNAPSHOT_SPAN_BYTES == R.SPAN_BYTES
    assert macro("C2S_SNAPSHOT_MAX_BLOCKS") == E.SNAPSHOT_MAX_BLOCKS == R.MAX_BLOCKS
    assert macro("C2S_SNAPSHOT_MAGIC") == E.SNAPSHOT_MAGIC == R.MAGIC
    assert macro("C2S_SNAPSHOT_VERSION") == E.SNAPSHOT_VERSION == R.VERSION
    assert macro("C2S_SNAPSHOT_STATUS_BYTES") == E.SNAPSHOT_STATUS_BYTES


def test_checksums_wrap_and_detect_damage():
    rng = np.random.default_rng(7)
    w = rng.integers(0, 1 << 32, 70001, dtype=np.uint32)
    w[:64] = 0xFFFFFFFF
    assert R.sums(w) == R.sums_wrapping(w)                                     # Python integers against wrapping uint64
    big = np.full(1 << 21, 0xFFFFFFFF, dtype=np.uint32)                        # s2 passes 2^64 here: the wrap is exercised
    assert sum(range(1, big.size + 1)) * 0xFFFFFFFF >= 1 << 64
    assert R.sums(big) == R.sums_wrapping(big) == (big.size * 0xFFFFFFFF % (1 << 64),
                                                   sum(range(1, big.size + 1)) * 0xFFFFFFFF % (1 << 64))
    s1, s2 = R.sums(w)
    flipped = w.copy()
    flipped[12345] ^= 1 << 9
    f1, f2 = R.sums(flipped)
    assert f1 != s1 and f2 != s2
    swapped = w.copy()
    assert swapped[100] != swapped[20100]
    swapped[100], swapped[20100] = w[20100], w[100]
    g1, g2 = R.sums(swapped)
    assert g1 == s1, "s1 cannot see a swap"
    assert g2 != s2, "s2 must"
    t1, t2 = R.sums(w[:-4])
    assert (t1, t2) != (s1, s2)
    blob = R.blob([w])
    assert R.check(blob, 1) == 0
    assert R.check(blob[:-16], 1) == 4                                         # a truncated payload: the size in the header
    cut = blob[:-16].copy()
    cut[16:24] = np.array([cut.size - 64], dtype=np.uint64).view(np.uint8)     # ... and, with the size forged, the sums
    assert R.check(cut, 1) == 5
    assert R.check(blob, 2) == 3
    bad = blob.copy()
    bad[64 + 4 * 777] ^= 4
    assert R.check(bad, 1) == 5


# ------------------------------------------------------------------------------------------------------- torch-format conversion
NAMES = ["a.weight", "a.bias", "b.weight", "c.weight"]
SHAPES = [(3, 5), (3,), (2, 2, 2), (7,)]
KEYS = ["a.weight", "a.bias", "a.running_mean", "a.num_batches_tracked", "b.weight", "c.weight"]
STEPS = [3, 3, 0, 5]


def _flat_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    offs, o = [], 0
    for s in SHAPES:
        offs.append(o)
        o += (int(np.prod(s)) + 3) // 4 * 4
    flats = [torch.zeros(o) for _ in range(3)]
    for i, (s, off) in enumerate(zip(SHAPES, offs)):
        n = int(np.prod(s))
        flats[0][off:off + n] = torch.randn(n, generator=g)
        if STEPS[i]:
            flats[1][off:off + n] = 0.1 * torch.randn(n, generator=g)
            flats[2][off:off + n] = 0.01 * torch.rand(n, generator=g) + 1e-4
    bufs = {"a.running_mean": torch.randn(3, generator=g), "a.num_batches_tracked": torch.tensor(11)}
    return offs, o, flats, bufs


def test_conversion_round_trip_is_the_identity():
    from crop2seg_amd import checkpoint as CK
    offs, total, flats, bufs = _flat_state()
    state = CK.flat_to_torch(KEYS, NAMES, SHAPES, offs, *flats, STEPS, bufs, lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    assert list(state["state_dict"]) == KEYS
    assert sorted(state["optimizer"]["state"]) == [0, 1, 3], "a step-0 parameter has no entry"
    st = state["optimizer"]["state"][3]["step"]
    assert torch.is_tensor(st) and st.dtype == torch.float32 and float(st) == 5.0
    skeleton = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]
    group = state["optimizer"]["param_groups"][0]
    assert set(group) == set(skeleton) and group["params"] == [0, 1, 2, 3]
    assert (group["lr"], tuple(group["betas"]), group["eps"]) == (2e-3, (0.8, 0.99), 1e-7)
    p, m, v, steps, b = CK.torch_to_flat(state, NAMES, SHAPES, offs, total)
    assert torch.equal(p, flats[0]) and torch.equal(m, flats[1]) and torch.equal(v, flats[2]) and steps == STEPS
    assert sorted(b) == sorted(bufs) and all(torch.equal(b[k], bufs[k]) for k in bufs)
    again = CK.flat_to_torch(KEYS, NAMES, SHAPES, offs, p, m, v, steps, b, lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    for k in KEYS:
        assert torch.equal(again["state_dict"][k], state["state_dict"][k])
    assert not CK.is_bit_exact(state)                                          # no key of our own yet: the reference's format


def test_conversion_lists_every_difference():
    from crop2seg_amd import checkpoint as CK
    offs, total, flats, bufs = _flat_state()
    state = CK.flat_to_torch(KEYS, NAMES, SHAPES, offs, *flats, STEPS, bufs)
    state["state_dict"]["a.bias"] = torch.zeros(4)
    del state["state_dict"]["c.weight"]
    with pytest.raises(ValueError) as e:
        CK.torch_to_flat(state, NAMES, SHAPES, offs, total)
    assert "a.bias" in str(e.value) and "c.weight" in str(e.value)


def test_torch_adam_accepts_the_state_and_steps_like_fp64_adam():
    """torch.optim.Adam over CPU parameters loads the converted optimiser state; one step with a fixed gradient equals a
    float64 restatement of Adam (bias correction from the loaded step count) within 1e-6 relative per parameter."""
    from crop2seg_amd import checkpoint as CK
    offs, total, flats, bufs = _flat_state(1)
    lr, (b1, b2), eps = 1e-3, (0.9, 0.999), 1e-8
    state = CK.flat_to_torch(KEYS, NAMES, SHAPES, offs, *flats, STEPS, bufs, lr=lr, betas=(b1, b2), eps=eps)
    params = [state["state_dict"][n].clone().requires_grad_(True) for n in NAMES]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps)
    opt.load_state_dict(state["optimizer"])
    g = torch.Generator().manual_seed(9)
    grads = [torch.randn(s, generator=g) for s in SHAPES]
    for p, gr in zip(params, grads):
        p.grad = gr.clone()
    opt.step()
    for i, (n, s, off) in enumerate(zip(NAMES, SHAPES, offs)):
        cnt = int(np.prod(s))
        p0 = flats[0][off:off + cnt].double()
        m0, v0, gr = flats[1][off:off + cnt].double(), flats[2][off:off + cnt].double(), grads[i].reshape(-1).double()
        t = STEPS[i] + 1
        m1, v1 = b1 * m0 + (1 - b1) * gr, b2 * v0 + (1 - b2) * gr * gr
        want = p0 - lr / (1 - b1 ** t) * m1 / (v1.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        err = float((params[i].detach().reshape(-1).double() - want).norm() / (want.norm() + 1e-30))
        assert err < 1e-6, (n, err)
        assert int(opt.state[params[i]]["step"]) == t


def test_reference_only_file_converts_and_is_flagged():
    """A checkpoint as the reference's train.py writes it: a real torch.optim.Adam state dict, no key of ours."""
    from crop2seg_amd import checkpoint as CK
    offs, total, flats, bufs = _flat_state(2)
    params = [torch.nn.Parameter(flats[0][o:o + int(np.prod(s))].reshape(s).clone()) for s, o in zip(SHAPES, offs)]
    opt = torch.optim.Adam(params, lr=1e-3)
    for _ in range(2):
        for p in params[:3]:                                                   # the last one never trains: no state entry
            p.grad = torch.ones_like(p)
        opt.step()
    sd = {n: p.detach().clone() for n, p in zip(NAMES, params)}
    sd.update(bufs)
    ckpt = {"epoch": 4, "best_mIoU": 0.5, "state_dict": sd, "optimizer": opt.state_dict()}
    assert not CK.is_bit_exact(ckpt)
    p, m, v, steps, b = CK.torch_to_flat(ckpt, NAMES, SHAPES, offs, total)
    assert steps == [2, 2, 2, 0]
    for i, (s, o) in enumerate(zip(SHAPES, offs)):
        n = int(np.prod(s))
        assert torch.equal(p[o:o + n], params[i].detach().reshape(-1))
        if steps[i]:
            assert torch.equal(m[o:o + n], opt.state[params[i]]["exp_avg"].reshape(-1))
            assert torch.equal(v[o:o + n], opt.state[params[i]]["exp_avg_sq"].reshape(-1))
        else:
            assert not m[o:o + n].any() and not v[o:o + n].any()
    assert torch.equal(b["a.running_mean"], bufs["a.running_mean"])
    with pytest.warns(UserWarning, match="not bit-exact"):
        CK.warn_not_bit_exact()


# ------------------------------------------------------------------------------------------------------- ABI
NEW = ["c2s_snapshot_job_bytes", "c2s_snapshot_job_blocks", "c2s_snapshot_job_fill", "c2s_snapshot_gather",
       "c2s_snapshot_verify", "c2s_snapshot_scatter"]


def test_new_entry_points_are_declared_bound_and_checked():
    from crop2seg_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c2s_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
    L = _lib.lib()
    assert L.c2s_abi_version() == 4
    assert L.c2s_snapshot_job_bytes() == 32
    assert [L.c2s_snapshot_job_blocks(n) for n in (0, 4, 8192, 8196, 8176, 8180)] == [0, 1, 1, 2, 1, 1]
    rec = ctypes.create_string_buffer(32)
    assert L.c2s_snapshot_job_fill(rec, 4096, 20, 32, 3) == 0
    assert np.frombuffer(rec.raw, dtype=np.int64).tolist() == [4096, 20, 32, 3]
    assert L.c2s_snapshot_job_fill(rec, None, 0, 0, 0) == 0                    # an empty region needs no address
    for bad in ((4096, 6, 0, 0), (4096, 4, 8, 0), (4098, 4, 0, 0), (None, 4, 0, 0), (4096, -4, 0, 0), (4096, 4, 0, -1)):
        assert L.c2s_snapshot_job_fill(rec, *bad) == -1, bad
    # the launchers check their arguments before they touch the device
    assert L.c2s_snapshot_gather(4096, 1, 4096, 60, None) == -1 and b"snapshot_gather" in L.c2s_last_error()
    assert L.c2s_snapshot_gather(4096, 1, 4100, 64, None) == -1
    assert L.c2s_snapshot_gather(4096, 0, 4096, 64, None) == -1
    assert L.c2s_snapshot_verify(4096, 72, 1, 4096, None) == -1
    assert L.c2s_snapshot_scatter(4096, 1, 4096, 64, None, None) == -1
