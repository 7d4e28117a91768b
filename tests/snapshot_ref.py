"""numpy restatement of the snapshot blob (include/c2s_hip.h, training-state snapshots): layout, header and the two
checksums, written from the header's text alone -- nothing here imports crop2seg_amd."""
import numpy as np

HEADER_BYTES = 64
SPAN_BYTES = 8192            # one workgroup's span
MAX_BLOCKS = 1024            # workgroups of one launch: the grid's first pass covers MAX_BLOCKS spans
MAGIC = int.from_bytes(b"C2SS", "little")
VERSION = 1


def layout(region_bytes):
    """(offsets from the payload's start, payload bytes): every region on a multiple of 16, padded to the next one."""
    offs, o = [], 0
    for n in region_bytes:
        assert n >= 0 and n % 4 == 0
        offs.append(o)
        o += -(-n // 16) * 16
    return offs, o


def block_starts(region_bytes):
    """First virtual block of every region: one block per span of the padded region."""
    out, b = [], 0
    for n in region_bytes:
        out.append(b)
        b += -(-(-(-n // 16) * 16) // SPAN_BYTES)
    return out


def sums(payload_words):
    """s1 = sum w_i, s2 = sum (i + 1) w_i mod 2^64, in Python integers (no wrap-around to trust)."""
    w = np.asarray(payload_words, dtype=np.uint32)
    if w.size == 0:
        return 0, 0
    s1 = int(w.astype(np.uint64).sum(dtype=np.uint64))            # < 2^32 * size: exact below 2^32 words
    # s2 in 2^16-word pieces whose partial sums stay below 2^64, reduced in Python integers
    s2 = 0
    step = 1 << 16
    for a in range(0, w.size, step):
        part = w[a:a + step].astype(np.uint64)
        local = np.arange(1, part.size + 1, dtype=np.uint64)
        s2 += int((local * part).sum(dtype=np.uint64)) + a * int(part.sum(dtype=np.uint64))
    return s1 % (1 << 64), s2 % (1 << 64)


def sums_wrapping(payload_words):
    """The same with numpy's wrapping uint64 arithmetic throughout."""
    w = np.asarray(payload_words, dtype=np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(w.sum(dtype=np.uint64)), int((np.arange(1, w.size + 1, dtype=np.uint64) * w).sum(dtype=np.uint64))


def blob(regions):
    """The whole blob as uint8 for regions given as numpy arrays of any 4- or 8-byte dtype."""
    raw = [np.ascontiguousarray(r).reshape(-1).view(np.uint8) for r in regions]
    offs, payload = layout([r.size for r in raw])
    out = np.zeros(HEADER_BYTES + payload, dtype=np.uint8)
    for r, o in zip(raw, offs):
        out[HEADER_BYTES + o:HEADER_BYTES + o + r.size] = r
    s1, s2 = sums(out[HEADER_BYTES:].view(np.uint32))
    head = np.zeros(HEADER_BYTES // 4, dtype=np.uint32)
    head[0], head[1], head[2] = MAGIC, VERSION, len(regions)
    head[4:6] = np.array([payload], dtype=np.uint64).view(np.uint32)
    head[6:8] = np.array([s1], dtype=np.uint64).view(np.uint32)
    head[8:10] = np.array([s2], dtype=np.uint64).view(np.uint32)
    out[:HEADER_BYTES] = head.view(np.uint8)
    return out


def check(blob_bytes, nregions):
    """What c2s_snapshot_verify decides: 0 fine, 1 magic, 2 version, 3 region count, 4 payload size, 5 a sum differs."""
    b = np.asarray(blob_bytes, dtype=np.uint8)
    head = b[:HEADER_BYTES].view(np.uint32)
    if head[0] != MAGIC:
        return 1
    if head[1] != VERSION:
        return 2
    if head[2] != nregions:
        return 3
    if int(head[4:6].view(np.uint64)[0]) != b.size - HEADER_BYTES:
        return 4
    s1, s2 = sums(b[HEADER_BYTES:].view(np.uint32))
    if (int(head[6:8].view(np.uint64)[0]), int(head[8:10].view(np.uint64)[0])) != (s1, s2):
        return 5
    return 0
