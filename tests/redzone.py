"""A guard-band allocator for the tests: every kernel output between poisoned red zones.

`with arena(device, nbytes) as a:` serves every allocation that torch's factory functions make on `device` (empty, zeros,
ones, full, their *_like and new_* forms, empty_strided with dense row-major strides, clone) from one buffer allocated
up front.  Nothing else changes: a block starts on a 512-byte boundary like a block of the caching allocator, it is
exactly numel * itemsize bytes long, and the launches are the ones the code under test makes anyway.  What changes is
the neighbourhood and the initial content:

- the whole buffer is filled once with the word POISON (a NaN as float32, -5921371 as int32, about -2.5e16 as int64,
  non-zero in every byte); `empty` leaves its block poisoned, `zeros` / `ones` / `full` / `clone` fill theirs;
- the byte after a block is guard band: at least `zone` bytes (64 KiB) lie between two blocks and in front of the first
  one, and the never-allocated rest of the buffer is guard band too;
- blocks are bump-allocated and never reused inside one `with`, so data pointers stay unique (the tape keys on them).

Checks: `assert_intact()` (every word outside the blocks still holds the poison; run by __exit__ unless an exception is
propagating) and `poisoned(t)` (which 4-byte words of a tensor still hold it).  A damaged guard band is reported with the
nearest block (index, shape, dtype), the byte offsets of the damaged words relative to that block's start and end, and
the allocation site: the innermost stack frame inside crop2seg_amd/ at allocation time.

Allocations for another device type, pinned ones, sparse layouts, empty tensors and non-contiguous *_like / clone
sources pass through to the ordinary allocator, and so does every tensor an operator other than a factory returns
(host <-> device copies, torch arithmetic in a test): inputs need not live in the arena.  `copies=True` is for runners
whose kernels write into tensors they made with `.cuda()`: a copy that arrives from another device type then gets a block
of its own too.

What it cannot see is listed in DESIGN.md (section 4): reads, and stores into slack that belongs to the block itself.
"""
import bisect
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

POISON = 0xFFA5A5A5                       # float32: NaN (sign 1, exponent 255, mantissa 0x25A5A5)
POISON_I32 = POISON - (1 << 32)           # -5921371
POISON_BYTES = (0xA5, 0xA5, 0xA5, 0xFF)   # little endian
ALIGN = 512                               # the caching allocator's block alignment
ZONE = 64 * 1024
_PKG = os.sep + "crop2seg_amd" + os.sep
_HERE = os.path.abspath(__file__)

aten = torch.ops.aten


class ArenaExhausted(RuntimeError):
    pass


class RedzoneError(AssertionError):
    pass


class Block:
    __slots__ = ("index", "off", "nbytes", "shape", "dtype", "site")

    def __init__(self, index, off, nbytes, shape, dtype, site):
        self.index, self.off, self.nbytes, self.shape, self.dtype, self.site = index, off, nbytes, shape, dtype, site

    def __repr__(self):
        return f"block {self.index} {tuple(self.shape)} {str(self.dtype).replace('torch.', '')} allocated at {self.site}"


def _round_up(n, a):
    return (n + a - 1) // a * a


def _site():
    """Innermost frame inside crop2seg_amd/, else the innermost one outside torch and this file."""
    f = sys._getframe(2)
    fallback = None
    while f is not None:
        name = f.f_code.co_filename
        if _PKG in name:
            return f"{name[name.rindex(_PKG) + 1:]}:{f.f_lineno} ({f.f_code.co_name})"
        if fallback is None and os.path.abspath(name) != _HERE and (os.sep + "torch" + os.sep) not in name:
            fallback = f"{os.path.basename(name)}:{f.f_lineno} ({f.f_code.co_name})"
        f = f.f_back
    return fallback or "?"


def _dense(t):
    return t.layout == torch.strided and t.is_contiguous()


def _full_dtype(v):
    if isinstance(v, bool):
        return torch.bool
    if isinstance(v, int):
        return torch.int64
    if isinstance(v, complex):
        return torch.complex64 if torch.get_default_dtype() == torch.float32 else torch.complex128
    return torch.get_default_dtype()


class Arena(TorchDispatchMode):
    def __init__(self, device, nbytes, zone=ZONE, copies=False):
        super().__init__()
        self.copies = bool(copies)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.zone = _round_up(max(int(zone), ALIGN), ALIGN)
        self.nbytes = _round_up(int(nbytes), ALIGN)
        raw = torch.empty(self.nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        lead = -raw.data_ptr() % ALIGN
        self._raw = raw
        self.buf = raw[lead:lead + self.nbytes]
        self.base = self.buf.data_ptr()
        self.words = self.buf.view(torch.int32)
        self.words.fill_(POISON_I32)
        self.blocks = []
        self._starts = []
        self.cursor = self.zone            # next block's offset; [0, zone) is the first guard band
        self.allocated = 0                 # payload bytes handed out

    # ---------------------------------------------------------------------------------------------
    # allocation
    # ---------------------------------------------------------------------------------------------
    @property
    def used(self):
        """Bytes of the arena consumed so far, guard bands included: what `nbytes` must be at least."""
        return self.cursor

    def _mine(self, device, pin_memory=False, layout=None):
        if pin_memory or layout not in (None, torch.strided):
            return False
        d = torch.device(device) if device is not None else torch.empty(0).device
        if d.type != self.device.type:
            return False
        return d.index is None or self.device.index is None or d.index == self.device.index

    def _alloc(self, shape, dtype):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nb = numel * dtype.itemsize
        off = self.cursor
        if off + nb + self.zone > self.nbytes:
            raise ArenaExhausted(f"arena of {self.nbytes} bytes exhausted: block {len(self.blocks)} {shape} {dtype} needs "
                                 f"{nb} bytes and its guard band at offset {off} ({self.allocated} payload bytes so far)")
        self.cursor = _round_up(off + nb + self.zone, ALIGN)
        self.allocated += nb
        self.blocks.append(Block(len(self.blocks), off, nb, shape, dtype, _site()))
        self._starts.append(off)
        return self.buf[off:off + nb].view(dtype).view(shape)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        h = _HANDLERS.get(func)
        if h is not None:
            out = h(self, args, kwargs)
            if out is not NotImplemented:
                return out
        return func(*args, **kwargs)

    def _factory(self, size, dtype, kwargs, fill=None):
        if not self._mine(kwargs.get("device"), kwargs.get("pin_memory"), kwargs.get("layout")):
            return NotImplemented
        if kwargs.get("memory_format") not in (None, torch.contiguous_format):
            return NotImplemented
        if any(int(s) == 0 for s in size):
            return NotImplemented
        t = self._alloc(size, dtype or torch.get_default_dtype())
        if fill is not None:
            t.fill_(fill)
        return t

    def _like(self, src, size, kwargs, fill=None, copy=False):
        device = kwargs.get("device") or src.device
        if not self._mine(device, kwargs.get("pin_memory"), kwargs.get("layout") or src.layout):
            return NotImplemented
        mf = kwargs.get("memory_format")
        if size is None:                      # *_like / clone: the source's strides are kept
            if mf not in (None, torch.preserve_format, torch.contiguous_format):
                return NotImplemented
            if mf is not torch.contiguous_format and not _dense(src):
                return NotImplemented
            size = src.shape
        if any(int(s) == 0 for s in size):
            return NotImplemented
        t = self._alloc(size, kwargs.get("dtype") or src.dtype)
        if copy:
            t.copy_(src)
        elif fill is not None:
            t.fill_(fill)
        return t

    def _to_copy(self, src, kwargs):
        """copies=True only: a copy from another device type (`.cuda()`, `torch.tensor(..., device=)`) lands in the arena."""
        device = kwargs.get("device")
        if (not self.copies or device is None or src.device.type == self.device.type or not _dense(src)
                or not self._mine(device, kwargs.get("pin_memory"), kwargs.get("layout") or src.layout)
                or kwargs.get("memory_format") not in (None, torch.preserve_format, torch.contiguous_format)
                or src.numel() == 0):
            return NotImplemented
        t = self._alloc(src.shape, kwargs.get("dtype") or src.dtype)
        t.copy_(src, non_blocking=bool(kwargs.get("non_blocking", False)))
        return t

    # ---------------------------------------------------------------------------------------------
    # checks
    # ---------------------------------------------------------------------------------------------
    def tensor(self, block):
        """A block as a tensor again (for poisoned() on a tensor the code under test keeps to itself)."""
        return self.buf[block.off:block.off + block.nbytes].view(block.dtype).view(block.shape)

    def unwritten(self, where=_PKG.strip(os.sep)):
        """[(block, words still poisoned)] of the blocks allocated at a site containing `where` whose 4-byte words are not
        all overwritten.  A float32 result that is legitimately this NaN bit for bit does not occur in the tests."""
        self._sync()
        out = []
        for b in self.blocks:
            if where in b.site and b.nbytes >= 4:
                n = b.nbytes // 4
                left = int((self.words[b.off // 4:b.off // 4 + n] == POISON_I32).sum())
                if left:
                    out.append((b, left))
        return out

    def contains(self, t):
        p = t.data_ptr()
        return t.device.type == self.device.type and self.base <= p < self.base + self.nbytes

    def block_of(self, t):
        """The block a tensor handed out by this arena starts in."""
        off = t.data_ptr() - self.base
        i = bisect.bisect_right(self._starts, off) - 1
        assert i >= 0 and off < self.blocks[i].off + max(self.blocks[i].nbytes, 1), "not a tensor of this arena"
        return self.blocks[i]

    @staticmethod
    def poisoned(t):
        """Mask of the 4-byte words of a contiguous tensor that still hold the poison (shape of `t` for 4-byte types)."""
        assert t.is_contiguous() and t.numel() * t.dtype.itemsize % 4 == 0
        if t.dtype.itemsize == 4:
            return t.view(torch.int32) == POISON_I32
        return t.reshape(-1).view(torch.int32) == POISON_I32

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def damage(self, limit=64):
        """Damaged guard-band words, grouped by the nearest block:
        [{"block": Block or None, "start": [byte offsets relative to the block's start], "end": [... to its end]}].
        Offset 0 from the end is the first byte behind the block; offsets from the start are negative in front of it."""
        self._sync()
        bad = self.words != POISON_I32
        tails = []
        for b in self.blocks:
            lo, hi = b.off // 4, (b.off + b.nbytes + 3) // 4
            bad[lo:hi] = False
            if b.nbytes % 4:
                tails.append(b)
        hits = [4 * int(i) for i in bad.nonzero().flatten()[:limit].cpu()]
        if tails:                           # a block that ends inside a word: the rest of that word is guard band
            for b in tails:
                end = b.off + b.nbytes
                rest = self.buf[end:_round_up(end, 4)].cpu().tolist()
                if rest != list(POISON_BYTES[end % 4:]):
                    hits.append(end)
        out = {}
        for p in sorted(set(hits)):
            blk, dist = None, None
            i = bisect.bisect_right(self._starts, p)
            for j in (i - 1, i):
                if 0 <= j < len(self.blocks):
                    b = self.blocks[j]
                    d = b.off - p if p < b.off else p + 4 - (b.off + b.nbytes)
                    if dist is None or d < dist:
                        blk, dist = b, d
            e = out.setdefault(blk.index if blk else -1, {"block": blk, "start": [], "end": []})
            e["start"].append(p - blk.off if blk else p)
            e["end"].append(p - (blk.off + blk.nbytes) if blk else p)
        return list(out.values())

    def assert_intact(self):
        found = self.damage()
        if not found:
            return
        lines = []
        for e in found:
            b = e["block"]
            if b is None:
                lines.append(f"words at arena offsets {e['start']} damaged, no block allocated")
                continue
            before = [s for s in e["start"] if s < 0]
            after = [x for s, x in zip(e["start"], e["end"]) if s >= 0]
            what = []
            if before:
                what.append(f"{len(before)} word(s) before its start, at bytes {before} from the start")
            if after:
                what.append(f"{len(after)} word(s) past its end, at bytes {['+%d' % x for x in after]} from the end "
                            f"(the block is {b.nbytes} bytes)")
            lines.append(f"{b}: " + "; ".join(what))
        raise RedzoneError("guard band damaged (first words only):\n  " + "\n  ".join(lines))

    def __exit__(self, exc_type, exc, tb):
        super().__exit__(exc_type, exc, tb)
        if exc_type is None:
            self.assert_intact()
        return False


def _size_factory(fill):
    def h(a, args, kw):
        return a._factory(args[0], kw.get("dtype"), kw, fill)
    return h


def _h_full(a, args, kw):
    return a._factory(args[0], kw.get("dtype") or _full_dtype(args[1]), kw, args[1])


def _h_empty_strided(a, args, kw):
    size, stride = [int(s) for s in args[0]], [int(s) for s in args[1]]
    expect, run = [], 1
    for s in reversed(size):
        expect.append(run)
        run *= max(s, 1)
    if any(st != ex for s, st, ex in zip(size, stride, reversed(expect)) if s > 1):
        return NotImplemented
    return a._factory(size, kw.get("dtype"), kw)


def _like(fill=None, copy=False):
    def h(a, args, kw):
        return a._like(args[0], None, kw, fill, copy)
    return h


def _h_full_like(a, args, kw):
    return a._like(args[0], None, kw, args[1])


def _new(fill=None):
    def h(a, args, kw):
        return a._like(args[0], args[1], kw, fill)
    return h


def _h_new_full(a, args, kw):
    return a._like(args[0], args[1], kw, args[2])


_HANDLERS = {
    aten.empty.memory_format: _size_factory(None),
    aten.zeros.default: _size_factory(0),
    aten.ones.default: _size_factory(1),
    aten.full.default: _h_full,
    aten.empty_strided.default: _h_empty_strided,
    aten.empty_like.default: _like(),
    aten.zeros_like.default: _like(0),
    aten.ones_like.default: _like(1),
    aten.full_like.default: _h_full_like,
    aten.new_empty.default: _new(),
    aten.new_zeros.default: _new(0),
    aten.new_ones.default: _new(1),
    aten.new_full.default: _h_new_full,
    aten.clone.default: _like(copy=True),
    aten._to_copy.default: lambda a, args, kw: a._to_copy(args[0], kw),
}


def arena(device, nbytes, zone=ZONE, copies=False):
    return Arena(device, nbytes, zone, copies)
