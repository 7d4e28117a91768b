"""The weight-gradient kernels at chosen slice counts: the table of kernel rows, the slice counts and frame patterns, float64
references per frame and per tile, and a float32 model of the split-K walk (CPU only, no GPU import).

Every weight gradient is split-K (csrc/conv_wgrad.hip): workgroup `slice` of `nslices` walks the position tiles
start(slice), start(slice) + nslices, ... over all frames, skips the tiles of padded frames, keeps its sums in registers and
writes one slab; the slice sum adds the slabs.  start(slice) is the slice itself, or in the tile and Winograd kernels, when
nslices is a multiple of 8, the XCD permutation (slice & 7) * (nslices / 8) + (slice >> 3).

ROWS holds one row per kernel instantiation c2s_conv_wgrad can launch (fifteen (family, K) pairs in seven families), each on
the smallest plane its plan (choose<K, S>) accepts, with enough frames that one slice walks six tiles or more and each of two
slices three or more; five more rows repeat the 64-channel 3x3 ones under zero padding (the F(2x3,3x3) kernels read a zero
halo there).  tile_grid() re-derives the tiling of each family from the same conditions.
"""
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from conv_ref import U


class Row(NamedTuple):
    id: str
    N: int
    chans: Tuple[int, ...]
    Cout: int
    H: int                        # input plane
    W: int
    K: int
    S: int
    pad: int
    mode: str                     # "reflect" | "zeros"
    force: Tuple[int, int]        # c2s_wgrad_algorithms(winograd_3x3, winograd_4x4s2) while the row runs
    family: int                   # the family c2s_wgrad_path must report (the table in include/c2s_hip.h)


AUTO, DIRECT = (-1, -1), (0, 0)
ROWS = [
    # F(2x2,3x3): 8 waves (input channels a multiple of 64) and 4 waves (two sources, 96 channels, padded Cout)
    Row("f23-8wave", 6, (64,), 64, 8, 32, 3, 1, 1, "reflect", AUTO, 5),
    Row("f23-4wave-two-sources", 6, (32, 64), 40, 8, 32, 3, 1, 1, "reflect", AUTO, 4),
    # three tile rows: the middle one touches neither edge of the plane and takes the 8-wave kernel's buffer loads (on 8 x 32
    # no tile does), here from two sources
    Row("f23-8wave-interior", 4, (32, 32), 64, 12, 32, 3, 1, 1, "reflect", AUTO, 5),
    # F(2x2,2x2) over the input parities
    Row("f22", 6, (32,), 64, 16, 64, 4, 2, 1, "reflect", AUTO, 6),
    # 32-wide tiles
    Row("tile32-3x3", 6, (16,), 24, 4, 32, 3, 1, 1, "reflect", AUTO, 1),
    Row("tile32-1x1", 6, (64,), 32, 8, 32, 1, 1, 0, "zeros", AUTO, 1),
    Row("tile32-4x4s2", 6, (8,), 72, 8, 64, 4, 2, 1, "zeros", AUTO, 1),
    Row("tile32-3x3-forced", 4, (64,), 64, 8, 32, 3, 1, 1, "reflect", DIRECT, 1),
    Row("tile32-4x4s2-forced", 4, (32,), 64, 16, 64, 4, 2, 1, "reflect", DIRECT, 1),
    # 16-wide tiles
    Row("tile16-3x3", 6, (32,), 64, 8, 16, 3, 1, 1, "reflect", AUTO, 2),
    Row("tile16-1x1", 6, (64,), 32, 16, 16, 1, 1, 0, "zeros", AUTO, 2),
    Row("tile16-4x4s2", 6, (64,), 64, 16, 32, 4, 2, 1, "reflect", AUTO, 2),
    # the first layer: MFMA rows are (tap, cin) pairs
    Row("first-10", 6, (10,), 64, 4, 32, 3, 1, 1, "reflect", AUTO, 3),
    Row("first-4-zeros", 6, (4,), 64, 4, 32, 3, 1, 1, "zeros", AUTO, 3),
    # the generic kernel: partial tiles both ways, planes narrower than a tile, every (K, S) it is built for
    Row("generic-3x3-ragged", 4, (24,), 40, 12, 40, 3, 1, 1, "reflect", AUTO, 0),
    Row("generic-3x3-8x8", 6, (64,), 64, 8, 8, 3, 1, 1, "reflect", AUTO, 0),
    Row("generic-1x1-4x4", 6, (64,), 32, 4, 4, 1, 1, 0, "zeros", AUTO, 0),
    Row("generic-4x4s2-ragged", 3, (8,), 72, 24, 80, 4, 2, 1, "reflect", AUTO, 0),
    Row("generic-2x2s2", 6, (16,), 64, 16, 16, 2, 2, 0, "zeros", AUTO, 0),
    Row("generic-6x6s2", 3, (16,), 64, 24, 24, 6, 2, 2, "reflect", AUTO, 0),          # three tap groups
    # zero-padded 3x3 with 64 channels: the F(2x3,3x3) kernels read a zero halo, the tile kernels mask instead of mirroring
    # (new rows go at the end: make_inputs seeds a row by its index)
    Row("f23-8wave-zeros", 6, (64,), 64, 8, 32, 3, 1, 1, "zeros", AUTO, 5),
    Row("f23-4wave-two-sources-zeros", 6, (32, 64), 40, 8, 32, 3, 1, 1, "zeros", AUTO, 4),
    Row("f23-8wave-interior-zeros", 4, (32, 32), 64, 12, 32, 3, 1, 1, "zeros", AUTO, 5),
    Row("tile32-3x3-zeros-forced", 4, (64,), 64, 8, 32, 3, 1, 1, "zeros", DIRECT, 1),
    Row("tile16-3x3-zeros", 6, (64,), 64, 8, 16, 3, 1, 1, "zeros", AUTO, 2),
]
# the instantiations of the switch in c2s_conv_wgrad
INSTANTIATIONS = {(0, 3), (0, 1), (0, 4), (0, 2), (0, 6), (1, 3), (1, 1), (1, 4), (2, 3), (2, 1), (2, 4), (3, 3), (4, 3),
                  (5, 3), (6, 4)}
# how a family rounds: the constants of the GPU test are per class
FAMILY_CLASS = ("direct",) * 4 + ("f23",) * 2 + ("f22",)

# 8 and 16 take the permuted start; 64 is more than any row's tile count (empty slabs must be zero); 3 and 5 leave uneven
# remainders
NSLICES = (1, 2, 3, 5, 8, 16, 64)
PATTERNS = ("none", "tail", "head", "all")


def out_plane(row):
    return (row.H + 2 * row.pad - row.K) // row.S + 1, (row.W + 2 * row.pad - row.K) // row.S + 1


def padded_frames(pattern, N):
    """The padded frames of a pattern.  "tail": a run in the middle of a walk and the last frame; "head": the first frame
    (the walk starts on a padded tile) and the last but one."""
    if pattern == "none":
        return []
    if pattern == "tail":
        return sorted({1, 2, N - 1})
    if pattern == "head":
        return sorted({0, N - 2})
    assert pattern == "all"
    return list(range(N))


def keep_mask(pattern, N):
    keep = torch.ones(N, dtype=torch.bool)
    keep[padded_frames(pattern, N)] = False
    return keep


def tile_grid(row):
    """(tile rows, tile columns, tiles down, tiles across) of the row's family in output positions, from the conditions of
    choose<K, S>: families 4 - 6 tile into 4 x 32; 1 - 3 into TP / TW x TW with TP = 128 (1x1) or 64 and TW = 32 or 16; the
    generic kernel into TP / PC x PC with TP = 64 (stride 2) or 128 and PC the largest power of two in 4 .. 32 that is not
    wider than the plane (partial tiles masked).
    The library is not asked (it reports the family, not the tiling): this is a copy of its rule, and the frame counts of
    ROWS (six tiles or more per row) are checked against the copy.  If the tile shapes of conv_wgrad.hip change, change them
    here too, or the rows may stop reaching the steady state of the pipelined loop while every test still passes."""
    Ho, Wo = out_plane(row)
    if row.family >= 4:
        th, tw = 4, 32
    elif row.family >= 1:
        tw = 16 if row.family == 2 else 32
        th = (128 if row.K == 1 else 64) // tw
    else:
        tw = 32
        while tw > 4 and tw > Wo:
            tw //= 2
        th = (64 if row.S == 2 else 128) // tw
    if row.family >= 1:
        assert Ho % th == 0 and Wo % tw == 0, row.id
    return th, tw, -(-Ho // th), -(-Wo // tw)


def ntiles(row):
    _, _, ty, tx = tile_grid(row)
    return row.N * ty * tx


def make_inputs(row, seed=0):
    """Finite x [N, Cin, H, W] and gout [N, Cout, Ho, Wo] (float32, CPU) of a row."""
    g = torch.Generator().manual_seed(seed + 1000 * ROWS.index(row))
    Ho, Wo = out_plane(row)
    return (torch.randn(row.N, sum(row.chans), row.H, row.W, generator=g),
            torch.randn(row.N, row.Cout, Ho, Wo, generator=g))


def _wgrad(row, x, gout):
    """Weight gradient [Cout, Cin, K, K] of the row's convolution at (x, gout), in their dtype: F.pad(reflect) + conv2d +
    autograd, as conv_ref.py."""
    w = torch.zeros(row.Cout, x.shape[1], row.K, row.K, dtype=x.dtype, requires_grad=True)
    if row.pad and row.mode == "reflect":
        y = F.conv2d(F.pad(x, (row.pad,) * 4, mode="reflect"), w, None, stride=row.S)
    else:
        y = F.conv2d(x, w, None, stride=row.S, padding=row.pad)
    y.backward(gout)
    return w.grad


def frame_refs(row, x, gout):
    """float64 weight gradient of every frame on its own, and the same map on absolute values: two tensors
    [N, Cout, Cin, K, K].  The reference of a frame pattern is their sum over the kept frames (pattern_ref)."""
    xd, gd = x.double(), gout.double()
    gw = torch.stack([_wgrad(row, xd[n:n + 1], gd[n:n + 1]) for n in range(row.N)])
    A = torch.stack([_wgrad(row, xd[n:n + 1].abs(), gd[n:n + 1].abs()) for n in range(row.N)])
    return gw, A


def pattern_ref(refs, keep):
    gw, A = refs
    return gw[keep].sum(0), A[keep].sum(0)


def tile_wgrads(row, x, gout, dtype):
    """The weight gradient of every tile on its own (gout zeroed outside the tile's rectangle), in tile order
    (frame, tile row, tile column): [ntiles, Cout, Cin, K, K] in `dtype`, and the frame of every tile."""
    th, tw, ty, tx = tile_grid(row)
    out, frames = [], []
    for n in range(row.N):
        for i in range(ty):
            for j in range(tx):
                g = torch.zeros_like(gout[n:n + 1], dtype=dtype)
                g[:, :, i * th:(i + 1) * th, j * tw:(j + 1) * tw] = gout[n:n + 1, :, i * th:(i + 1) * th, j * tw:(j + 1) * tw]
                out.append(_wgrad(row, x[n:n + 1].to(dtype), g))
                frames.append(n)
    return torch.stack(out), frames


def walk(row, slice_, nslices, nt):
    """The tiles workgroup `slice_` visits, padded or not, in order."""
    start = slice_
    if row.family >= 1 and nslices % 8 == 0:
        start = (slice_ & 7) * (nslices >> 3) + (slice_ >> 3)
    return list(range(start, nt, nslices))


MUTATIONS = ("drop-last-tile", "drop-tile-after-skip", "tile-twice", "padded-frame-included", "slab-left-out",
             "stale-empty-slab")


def splitk_model(row, tiles32, frames, keep, nslices, mutation=None):
    """float32 model of the split-K weight gradient: the tiles (tile_wgrads in float32, of finite inputs) dealt to `nslices`
    slabs as the kernels walk them, the tiles of padded frames skipped, each slab summed in walk order and the slabs summed
    in slice order.  `mutation`: one of MUTATIONS, applied at the first place it fits; returns (result, applied)."""
    nt = len(frames)
    slabs = torch.zeros((nslices,) + tuple(tiles32.shape[1:]), dtype=torch.float32)
    filled = [False] * nslices
    applied = False
    for s in range(nslices):
        visited = walk(row, s, nslices, nt)
        todo = [(t, i > 0 and not bool(keep[frames[visited[i - 1]]])) for i, t in enumerate(visited) if bool(keep[frames[t]])]
        if mutation == "padded-frame-included" and not applied and len(todo) < len(visited):
            todo, applied = [(t, False) for t in visited], True
        if mutation == "drop-last-tile" and not applied and todo:
            todo, applied = todo[:-1], True
        if mutation == "drop-tile-after-skip" and not applied and any(after for _, after in todo):
            i = [after for _, after in todo].index(True)
            todo, applied = todo[:i] + todo[i + 1:], True
        if mutation == "tile-twice" and not applied and todo:
            todo, applied = todo + todo[-1:], True
        for t, _ in todo:
            slabs[s] += tiles32[t]
            filled[s] = True
    if mutation == "stale-empty-slab" and not all(filled) and any(filled):
        slabs[filled.index(False)] = slabs[filled.index(True)]
        applied = True
    total = torch.zeros(tuple(tiles32.shape[1:]), dtype=torch.float32)
    for s in range(nslices):
        if mutation == "slab-left-out" and not applied and filled[s]:
            applied = True
            continue
        total += slabs[s]
    return total, applied


def model_constant(row, nslices):
    """c of |model - ref64| <= c * u * A for the float32 model, whatever the order inside a tile: an element is a sum of at
    most `positions per tile` products per tile (each rounded once), then at most `tiles per slice` additions into the slab
    and `nslices` additions of slabs; the error of n roundings in a sum of terms is below n * u * (sum of magnitudes) (to
    first order; the 2 covers the rest)."""
    th, tw, _, _ = tile_grid(row)
    return th * tw + -(-ntiles(row) // nslices) + nslices + 2


__all__ = ["U", "Row", "ROWS", "INSTANTIATIONS", "FAMILY_CLASS", "NSLICES", "PATTERNS", "MUTATIONS", "out_plane",
           "padded_frames", "keep_mask", "tile_grid", "ntiles", "make_inputs", "frame_refs", "pattern_ref", "tile_wgrads",
           "walk", "splitk_model", "model_constant"]
