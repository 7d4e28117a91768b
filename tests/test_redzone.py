"""The guard-band arena of tests/redzone.py, tested on the CPU: interception, layout, poison, the failure report for planted
out-of-bounds writes, poisoned() for planted unwritten elements, and one planted-fault demonstration (a "kernel" that an
ordinary comparison passes and the arena fails)."""
import struct

import pytest
import torch

import redzone as RZ

MB = 1 << 20


def _inside(a, t):
    off = t.data_ptr() - a.base
    return 0 <= off and off + t.numel() * t.dtype.itemsize <= a.nbytes


def test_poison_word_reads_as_the_module_says():
    w = struct.pack("<I", RZ.POISON)
    assert struct.unpack("<f", w)[0] != struct.unpack("<f", w)[0]            # NaN as float32
    assert struct.unpack("<i", w)[0] == RZ.POISON_I32 < -(1 << 22)
    assert struct.unpack("<q", w + w)[0] < -(1 << 54)
    assert all(b != 0 for b in w) and tuple(w) == RZ.POISON_BYTES
    assert torch.tensor([RZ.POISON_I32], dtype=torch.int32).view(torch.bfloat16).isnan()[1]


FACTORIES = [
    ("empty", lambda: torch.empty(5, 7), (5, 7), torch.float32, None),
    ("empty-i64", lambda: torch.empty(3, dtype=torch.int64), (3,), torch.int64, None),
    ("empty-u8", lambda: torch.empty(1027, dtype=torch.uint8), (1027,), torch.uint8, None),
    ("empty-bf16", lambda: torch.empty(9, dtype=torch.bfloat16), (9,), torch.bfloat16, None),
    ("empty-device", lambda: torch.empty(2, 3, device="cpu", dtype=torch.float32), (2, 3), torch.float32, None),
    ("empty_strided", lambda: torch.empty_strided((2, 3), (3, 1)), (2, 3), torch.float32, None),
    ("zeros", lambda: torch.zeros(4, 3, dtype=torch.int32), (4, 3), torch.int32, 0),
    ("ones", lambda: torch.ones(6), (6,), torch.float32, 1),
    ("full", lambda: torch.full((3, 3), 2.5), (3, 3), torch.float32, 2.5),
    ("full-int", lambda: torch.full((3,), 7), (3,), torch.int64, 7),
    ("empty_like", lambda: torch.empty_like(torch.ones(2, 5, dtype=torch.float64)), (2, 5), torch.float64, None),
    ("empty_like-dtype", lambda: torch.empty_like(torch.ones(2, 5), dtype=torch.int32), (2, 5), torch.int32, None),
    ("zeros_like", lambda: torch.zeros_like(torch.ones(7)), (7,), torch.float32, 0),
    ("ones_like", lambda: torch.ones_like(torch.zeros(7)), (7,), torch.float32, 1),
    ("full_like", lambda: torch.full_like(torch.zeros(2, 2), 3.0), (2, 2), torch.float32, 3.0),
    ("new_empty", lambda: torch.ones(2).new_empty(4, 4), (4, 4), torch.float32, None),
    ("new_zeros", lambda: torch.ones(2).new_zeros(5), (5,), torch.float32, 0),
    ("new_ones", lambda: torch.ones(2, dtype=torch.int32).new_ones(5), (5,), torch.int32, 1),
    ("new_full", lambda: torch.ones(2).new_full((3,), 9.0), (3,), torch.float32, 9.0),
]


@pytest.mark.parametrize("name,make,shape,dtype,value", FACTORIES, ids=[f[0] for f in FACTORIES])
def test_factories_allocate_from_the_arena(name, make, shape, dtype, value):
    with RZ.arena("cpu", MB) as a:
        first = torch.empty(1)                     # so that the block under test has a predecessor
        t = make()
        assert _inside(a, first) and _inside(a, t), name
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert t.data_ptr() % RZ.ALIGN == 0
        b = a.block_of(t)
        assert b is a.blocks[-1] and b.nbytes == t.numel() * dtype.itemsize and b.shape == shape and b.dtype == dtype
        assert b.off - (a.blocks[-2].off + a.blocks[-2].nbytes) >= RZ.ZONE
        assert "test_redzone.py" in b.site
        if value is None:
            raw = a.buf[b.off:b.off + b.nbytes]
            assert raw.tolist() == [RZ.POISON_BYTES[i % 4] for i in range(b.nbytes)], "empty must stay poisoned"
            if dtype.itemsize >= 4:
                assert bool(a.poisoned(t).all())
            if dtype == torch.float32:
                assert bool(t.isnan().all())
        else:
            assert bool((t == value).all())
    assert a.allocated >= t.numel() * dtype.itemsize and a.used >= a.allocated + 3 * RZ.ZONE


def test_clone_copies_into_the_arena():
    src = torch.arange(12.0).view(3, 4)
    with RZ.arena("cpu", MB) as a:
        c = src.clone()
        assert _inside(a, c) and torch.equal(c, src) and not _inside(a, src)


def test_blocks_are_never_reused_and_pointers_are_unique():
    with RZ.arena("cpu", 4 * MB) as a:
        ptrs = set()
        for _ in range(20):
            t = torch.empty(100)
            ptrs.add(t.data_ptr())
            del t
        assert len(ptrs) == 20 and len(a.blocks) == 20


def test_pass_through_cases_are_untouched():
    base = torch.ones(4, 6)
    with RZ.arena("cpu", MB) as a:
        meta = torch.empty(3, device="meta")
        like_t = torch.empty_like(base.t())                       # non-contiguous source
        clone_t = base.t().clone()
        cl = torch.empty(1, 2, 3, 3, memory_format=torch.channels_last)
        none = torch.empty(0)
        arith = base + 1                                          # not a factory
        conv = base.to(torch.float64)
        assert meta.device.type == "meta" and like_t.stride() == (1, 6) and clone_t.stride() == (1, 6)
        assert cl.is_contiguous(memory_format=torch.channels_last) and none.numel() == 0
        for t in (like_t, clone_t, cl, arith, conv):
            assert not a.contains(t)
        assert len(a.blocks) == 0
        # a contiguous clone of a non-contiguous source is a fresh dense tensor: arena
        dense = base.t().clone(memory_format=torch.contiguous_format)
        assert a.contains(dense) and torch.equal(dense, base.t())
    with RZ.arena("cpu", MB) as a:
        if torch.cuda.is_available():
            assert not a.contains(torch.empty(3, device="cuda"))
            assert not a.contains(torch.empty(3).pin_memory())
    t = torch.empty(8)                                            # after the with: the ordinary allocator again
    assert not a.contains(t)


def test_exhaustion_raises_from_the_allocation():
    with pytest.raises(RZ.ArenaExhausted, match="exhausted"):
        with RZ.arena("cpu", 256 * 1024):
            torch.empty(10)                                       # fits: 64 KiB in front, 64 KiB behind
            torch.empty(32 * 1024)                                # 128 KiB payload does not
    with RZ.arena("cpu", 256 * 1024) as a:
        torch.empty(10)
        assert a.used == RZ.ZONE + RZ.ALIGN + RZ.ZONE


def _one(found):
    assert len(found) == 1, found
    return found[0]


def _past(t, first, count):
    """View of `count` elements starting `first` elements from t's first one, inside t's storage (the arena buffer)."""
    return t.as_strided((count,), (1,), t.storage_offset() + first)


def test_write_one_element_past_the_end_is_reported():
    a = RZ.arena("cpu", MB)
    with pytest.raises(RZ.RedzoneError) as err:
        with a:
            torch.zeros(16)
            t = torch.zeros(5, 3)
            torch.zeros(16)
            _past(t, 15, 1).fill_(1.0)
    e = _one(a.damage())
    assert e["block"].index == 1 and e["start"] == [60] and e["end"] == [0]
    msg = str(err.value)
    assert "block 1 (5, 3) float32" in msg and "test_redzone.py" in msg and "past its end" in msg and "'+0'" in msg


def test_write_one_element_before_the_start_is_reported():
    a = RZ.arena("cpu", MB)
    with pytest.raises(RZ.RedzoneError, match=r"block 1 \(7,\) int32.*before its start.*\[-4\]"):
        with a:
            torch.zeros(16)
            t = torch.zeros(7, dtype=torch.int32)
            _past(t, -1, 1).fill_(3)
    e = _one(a.damage())
    assert e["block"].index == 1 and e["start"] == [-4] and e["end"] == [-32]


def test_float4_over_a_ragged_end_is_reported():
    a = RZ.arena("cpu", MB)
    with pytest.raises(RZ.RedzoneError, match=r"block 0 \(6,\) float32"):
        with a:
            t = torch.zeros(6)
            _past(t, 4, 4).copy_(torch.ones(4))                   # one float4 at elements 4..7 of 6
    e = _one(a.damage())
    assert e["block"].index == 0 and e["end"] == [0, 4] and e["start"] == [24, 28]


def test_write_into_the_middle_of_another_blocks_guard_band_is_reported():
    a = RZ.arena("cpu", MB)
    with pytest.raises(RZ.RedzoneError):
        with a:
            t0 = torch.zeros(8)
            t1 = torch.zeros(8)
            torch.zeros(8)
            _past(t0, (t1.data_ptr() - t0.data_ptr()) // 4 + 8 + 4096, 2).fill_(0.0)      # 16 KiB behind t1, written from t0
    e = _one(a.damage())
    assert e["block"].index == 1 and e["end"] == [16384, 16388]


def test_odd_byte_length_block_guards_the_rest_of_its_word():
    a = RZ.arena("cpu", MB)
    with pytest.raises(RZ.RedzoneError, match=r"block 0 \(5,\) uint8"):
        with a:
            t = torch.zeros(5, dtype=torch.uint8)
            _past(t, 5, 1).fill_(0)
    assert _one(a.damage())["end"] == [0]
    with RZ.arena("cpu", MB):                                     # ... and writing all 5 bytes is clean
        torch.empty(5, dtype=torch.uint8).fill_(0)


def test_clean_run_reports_nothing():
    with RZ.arena("cpu", 2 * MB) as a:
        x = torch.empty(33, 5)
        x.copy_(torch.randn(33, 5))
        y = torch.empty_like(x)
        torch.mul(x, 2.0, out=y)
        z = torch.zeros(3, dtype=torch.int64)
        z += 1
        a.assert_intact()
        assert a.damage() == []
    assert a.damage() == []


def test_no_check_while_an_exception_propagates():
    with pytest.raises(KeyError):
        with RZ.arena("cpu", MB):
            t = torch.zeros(4)
            _past(t, 4, 1).fill_(1.0)
            raise KeyError("the runner's own failure wins")


def test_poisoned_finds_an_unwritten_corner():
    with RZ.arena("cpu", MB) as a:
        out = torch.empty(40, 19)
        full = torch.empty(40, 19)
        src = torch.randn(40, 19)
        full.copy_(src)
        out[:32].copy_(src[:32])
        out[32:, :16].copy_(src[32:, :16])                         # an 8 x 3 corner (rows 32.., columns 16..) is never stored
        m = a.poisoned(out)
        assert m.shape == out.shape and int(m.sum()) == 24 and bool(m[32:, 16:].all())
        assert not bool(a.poisoned(full).any())
        i64 = torch.empty(4, dtype=torch.int64)
        i64[:3] = 5
        assert a.poisoned(i64).tolist() == [False] * 6 + [True] * 2


def test_unwritten_lists_blocks_by_allocation_site():
    with RZ.arena("cpu", MB) as a:
        done = torch.empty(6, 4)
        done.copy_(torch.ones(6, 4))
        part = torch.empty(6, 4)
        part[:4] = 1.0
        short = torch.empty(3, dtype=torch.uint8)                   # under one word: never listed
        left = a.unwritten("test_redzone.py")
        assert [(b, n) for b, n in left] == [(a.block_of(part), 8)] and a.unwritten() == []     # (none made in crop2seg_amd/)
        again = a.tensor(left[0][0])
        assert again.data_ptr() == part.data_ptr() and again.shape == part.shape and bool(a.poisoned(again)[4:].all())
        assert a.block_of(short).nbytes == 3


def test_copies_stay_outside_unless_asked():
    src = torch.arange(4.0)
    with RZ.arena("cpu", MB) as a:
        assert not a.contains(src.to(torch.float64)) and not a.contains(src.to("cpu", copy=True))
    with RZ.arena("cpu", MB, copies=True) as a:                     # same device type: still no block
        assert not a.contains(src.to(torch.float64)) and len(a.blocks) == 0


def _copy_rows_in_quads(dst, src, rows):
    """A planted fault: copies `rows` rows of `src` four at a time, as a kernel with a 4-row tile and no tail predicate would,
    so the last quad runs past `rows`.  `dst` is addressed as raw memory from its first element."""
    W = src.shape[1]
    for r0 in range(0, rows, 4):
        quad = src[r0:r0 + 4]
        if quad.shape[0] < 4:
            quad = torch.cat([quad, torch.zeros(4 - quad.shape[0], W)])
        _past(dst, r0 * W, 4 * W).copy_(quad.reshape(-1))


def test_planted_fault_passes_a_comparison_and_fails_in_the_arena():
    src = torch.randn(10, 6)                                       # 10 rows: not a multiple of 4
    # outside the arena: the overrun lands in slack behind `dst` (here: the rest of a larger storage, as the caching
    # allocator's rounding provides on the device), and the comparison with the reference passes
    slab = torch.empty(12 * 6 + 64)
    dst = slab[:60].view(10, 6)
    _copy_rows_in_quads(dst, src, 10)
    assert torch.equal(dst, src)
    a = RZ.arena("cpu", MB)
    with pytest.raises(RZ.RedzoneError, match=r"block 0 \(10, 6\) float32"):
        with a:
            dst = torch.empty(10, 6)
            _copy_rows_in_quads(dst, src, 10)
            assert torch.equal(dst, src)                           # the result is still right
    e = _one(a.damage())
    assert e["end"] == [4 * i for i in range(12)]                  # rows 10 and 11: 12 floats behind the block
