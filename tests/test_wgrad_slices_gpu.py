"""The weight-gradient kernels of csrc/conv_wgrad.hip at chosen slice counts, and the slice sums, against float64 per element.

The engine derives `nslices` from the tile count and the CU count (engine._wgrad_slices), so at the small shapes of the other
per-element tests every slice holds one tile at most.  (For the F(2x2,2x2) family it counts tiles of 64 positions where the
kernel uses 128, so it asks for twice as many slices as there are tiles and half of the slabs are empty.)  Here the
descriptor is the engine's (engine._wgrad_desc, from the tensors that are passed) with `nslices` alone overridden, so that a
slice walks many tiles: the steady state of the pipelined loop (a register-staged tile committed while the next one is in
flight), padded frames met at the start, in the middle and at the end of a walk, odd slice counts, uneven remainders, the
XCD-permuted start (8, 16) and more slices than tiles (64: the empty slabs must be zero).

- one test per row of wgrad_ref.ROWS (one row per kernel instantiation): every nslices of wgrad_ref.NSLICES with the frame
  patterns none (null `valid`), tail and head, all frames padded at nslices = 3, one accumulating run on a random prior;
  padded frames hold NaN in x and gout;
- the slab workspace sits 64 floats into a sentinel buffer and `dst` is a window of another: the floats around them must be
  bit-unchanged;
- every result is finite, meets conv_ref.FROB_GRAD and |got - ref64| <= c * u * A element by element, and the same call
  twice gives the same bits;
- the slice sums on synthetic slabs (NaN in the padded channel rows and columns) for every tail of the 16-way loop, three
  destination layouts, with and without accumulation: |got - sum64| <= nslices * u * sum |slab|, which holds for any order;
- the batched slice sum against the per-job one, bit for bit.

Error constants c per class (how the family rounds): about 4x the worst ratio max |err| / (u * A) observed over the whole
table on an MI355X (printed with -s by test_reached_instantiations_are_the_table), capped at 1024; an indexing or
accumulation bug lands near 1/u ~ 1e7.  Slices here run chains of up to 36 tiles, so the constants of
test_conv_paths_gpu.py are not copied.  Observed worst ratios:

    direct 4.94   f23 2.47   f22 3.23

(the five zero-padded 3x3 rows added later: direct 3.51, f23 3.45)

The tests can fail.  Three local builds of the library (not part of the project), each changing arithmetic only, one per
loop; "existing" are the 165 convolution tests of test_conv_paths_gpu.py, test_conv_modes_gpu.py,
test_strided_geometry_gpu.py and test_ops_gpu.py:

- the generic loop skips the MFMAs of the third tile of a walk: the six generic rows fail (Frobenius error 0.2 - 0.4 at
  nslices = 1), the other rows and the slice-sum tests pass; all existing tests pass;
- the pipelined tile, F(2x2,3x3) and F(2x2,2x2) loops scale the gradient operand of the third tile a workgroup visits by 0:
  the fourteen rows of families 1 - 6 fail, the six generic rows pass; of the existing tests only
  test_first_layer_persistent_loop (640 tiles on 512 workgroups) fails;
- the slice sum drops the fourth partial sum of every lane (the slices 12 + q, 28 + q, ... of lane q): the synthetic slabs
  fail at every nslices >= 13 (13 of 21 cases) and sixteen rows fail (all but the four generic rows of 12 tiles or fewer,
  whose slabs 12 - 15 are empty); 62 of the existing tests fail too, the engine's slice counts being mostly above 12.
"""
import ctypes
import types

import pytest
import torch

import conv_ref as R
import wgrad_ref as G

pytestmark = pytest.mark.gpu

C_CLASS = {"direct": 20, "f23": 10, "f22": 13}
OBSERVED = {}            # class -> worst ratio over the rows that ran
REACHED = {}             # row id -> (family, K)
SENTINEL = 1234.5
GUARD = 64               # floats in front of and behind the slab workspace and the destination
CTX = types.SimpleNamespace(cus=256)          # what engine._wgrad_desc reads of a context; nslices is overridden


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _bits(t):
    return t.view(torch.int32)


def _guarded(n, fill=SENTINEL):
    """A sentinel buffer of GUARD + n + GUARD floats and its window of n floats."""
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n]


def _assert_guards(what, buf, n):
    want = torch.full((GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    assert torch.equal(_bits(buf[:GUARD]), _bits(want)), f"{what}: the floats in front were written"
    assert torch.equal(_bits(buf[GUARD + n:]), _bits(want)), f"{what}: the floats behind were written"


class _Case:
    """One row on the device: the sources and gout of every frame pattern, and the float64 references per frame."""

    def __init__(self, row):
        E, L = _engine()
        self.row, self.E = row, E
        self.pm = L.PAD_REFLECT if row.mode == "reflect" else L.PAD_ZEROS
        self.Ho, self.Wo = G.out_plane(row)
        self.Cin, self.KK = sum(row.chans), row.K * row.K
        x, gout = G.make_inputs(row)
        self.refs = G.frame_refs(row, x, gout)
        self.dev = {}
        for pattern in G.PATTERNS:
            keep = G.keep_mask(pattern, row.N)
            xp, gp = x.clone(), gout.clone()
            xp[~keep] = float("nan")
            gp[~keep] = float("nan")
            srcs, lo = [], 0
            for c in row.chans:
                srcs.append(xp[:, lo:lo + c].contiguous().cuda())
                lo += c
            self.dev[pattern] = (srcs, gp.cuda(), None if pattern == "none" else keep.int().cuda(), keep)
        g = torch.Generator().manual_seed(7)
        self.prior = torch.randn(row.Cout, self.Cin, row.K, row.K, generator=g)

    def run(self, nslices, pattern, accumulate=0):
        """c2s_conv_wgrad + c2s_wgrad_reduce as engine._wgrad_launch calls them, with d.nslices overridden and guards around
        the slab workspace and the destination.  Returns the weight gradient [Cout, Cin, K, K] (device)."""
        E, row = self.E, self.row
        what = f"{row.id} nslices {nslices} pattern {pattern}" + (" accumulate" if accumulate else "")
        srcs, gout, valid, _ = self.dev[pattern]
        d = E._wgrad_desc(CTX, srcs, row.Cout, self.Ho, self.Wo, row.K, row.S, row.pad, self.pm)
        d.nslices = nslices
        fam = ctypes.c_int(-1)
        assert E.lib().c2s_wgrad_path(ctypes.byref(d), ctypes.byref(fam)) == 0, E.lib().c2s_last_error()
        assert fam.value == row.family, f"{what}: family {fam.value}, the table says {row.family}"
        REACHED[row.id] = (fam.value, row.K)
        nfl = E.lib().c2s_wgrad_workspace_floats(ctypes.byref(d))
        sbuf, slabs = _guarded(nfl)
        nw = row.Cout * self.Cin * self.KK
        dbuf, dst = _guarded(nw)
        if accumulate:
            dst.copy_(self.prior.flatten())
        s1 = srcs[1] if len(srcs) > 1 else None
        E.check(E.lib().c2s_conv_wgrad(ctypes.byref(d), srcs[0].data_ptr(), E._ptr(s1), gout.data_ptr(), slabs.data_ptr(), nfl,
                                       E._ptr(valid), E._stream()), "conv_wgrad")
        E.check(E.lib().c2s_wgrad_reduce(ctypes.byref(d), slabs.data_ptr(), dst.data_ptr(), self.Cin * self.KK, self.KK,
                                         E._tap_array(list(range(self.KK))), accumulate, E._stream()), "wgrad_reduce")
        torch.cuda.synchronize()
        _assert_guards(f"{what}: slab workspace", sbuf, nfl)
        _assert_guards(f"{what}: destination", dbuf, nw)
        return dst.view(row.Cout, self.Cin, row.K, row.K).clone()

    def check(self, nslices, pattern, accumulate=0):
        row = self.row
        what = f"{row.id} nslices {nslices} pattern {pattern}" + (" accumulate" if accumulate else "")
        got = self.run(nslices, pattern, accumulate)
        again = self.run(nslices, pattern, accumulate)
        assert torch.equal(_bits(got), _bits(again)), f"{what}: the same call twice gives different bits"
        got = got.cpu()
        assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
        if pattern == "all":
            want = self.prior if accumulate else torch.zeros_like(got)
            assert torch.equal(_bits(got), _bits(want)), f"{what}: all frames padded must leave " + \
                ("the prior bit-identical" if accumulate else "exactly 0")
            return 0.0
        ref, A = G.pattern_ref(self.refs, self.dev[pattern][3])
        if accumulate:
            ref, A = ref + self.prior.double(), A + self.prior.double().abs()
        cls = G.FAMILY_CLASS[row.family]
        ratio = R.bound_ratio(got, ref, A)
        print(f"  {what}: {cls} {ratio:.2f}")
        OBSERVED[cls] = max(OBSERVED.get(cls, 0.0), ratio)
        R.assert_within(what, got, ref, A, C_CLASS[cls], R.FROB_GRAD)
        return ratio


def _run_row(row):
    E, _ = _engine()
    E.Workspace(torch.device("cuda"))          # one-time device initialisation (dynamic-LDS limits), as every context does
    try:
        E.lib().c2s_wgrad_algorithms(*row.force)
        case = _Case(row)
        print(f"\n{row.id}: family {row.family}, {G.ntiles(row)} tiles")
        for nslices in G.NSLICES:
            for pattern in ("none", "tail", "head"):
                case.check(nslices, pattern)
        case.check(3, "all")
        case.check(3, "tail", accumulate=1)
        case.check(3, "all", accumulate=1)
    finally:
        E.lib().c2s_wgrad_algorithms(-1, -1)


@pytest.mark.parametrize("row", G.ROWS, ids=[r.id for r in G.ROWS])
def test_wgrad_row(row):
    _run_row(row)


# =================================================================================================
# slice sums on synthetic slabs
# =================================================================================================
# the tails of the 16-way loop (k + 12 < nslices, then steps of 4 per lane): of one to three steps before the loop has run
# (12 and 13 give every lane three) and after it; after it a tail of three steps needs nslices - 16 in 9 + q .. 12 + q for lane
# q: 27 and 28 give it to lanes 0 - 2, 31 to lane 3
REDUCE_NSLICES = (1, 2, 3, 4, 5, 7, 8, 12, 13, 16, 17, 19, 20, 27, 28, 31, 32, 33, 35, 48, 49)


def _reduce_desc(Cin, Cout, K, S, nslices):
    """The engine's descriptor for a layer of these channel counts (the slice sums read its channel counts, kernel size and
    nslices only), nslices overridden."""
    E, L = _engine()
    pad = 0 if K == 1 else 1
    d = E._wgrad_desc(CTX, [torch.empty(1, Cin, 4 * S, 4 * S, device="meta")], Cout, 4, 4, K, S, pad, L.PAD_ZEROS)
    d.nslices = nslices
    return d


def _slabs(d, Cin, Cout, K, nslices, gen):
    """Random slabs [slice][tap][CinP][CoutB] with NaN in the padded channel rows and columns, behind and in front of
    guards; the buffer, its window and the CPU copy of the live part [slice][tap][Cin][Cout]."""
    E, _ = _engine()
    CinP, CoutB = -(-Cin // 32) * 32, -(-Cout // 64) * 64
    nfl = E.lib().c2s_wgrad_workspace_floats(ctypes.byref(d))
    assert nfl == nslices * K * K * CinP * CoutB
    live = torch.randn(nslices, K * K, Cin, Cout, generator=gen)
    full = torch.full((nslices, K * K, CinP, CoutB), float("nan"))
    full[:, :, :Cin, :Cout] = live
    buf, win = _guarded(nfl)
    win.copy_(full.flatten())
    return buf, win, live


def _layouts(Cin, Cout, K):
    """(name, floats of the destination buffer, offset, so, sc, taps) of the three destinations."""
    KK = K * K
    return [
        ("conv", Cout * Cin * KK, 0, Cin * KK, KK, list(range(KK))),
        # engine.conv_transpose2d: so = Cout * K * K; the rows of channels Cin .. Cout - 1 are not this job's
        ("transposed", Cout * Cout * KK, 0, Cout * KK, KK, list(range(KK))),
        # a strided, offset window, taps in reverse
        ("window", 17 + Cout * (Cin * (KK + 2) + 13), 17, Cin * (KK + 2) + 13, KK + 2, list(range(KK - 1, -1, -1))),
    ]


def _dst_index(Cin, Cout, K, off, so, sc, taps):
    o = torch.arange(Cout).view(1, 1, Cout)
    c = torch.arange(Cin).view(1, Cin, 1)
    t = torch.tensor(taps).view(K * K, 1, 1)
    return off + o * so + c * sc + t          # [tap][Cin][Cout], as a slab


@pytest.mark.parametrize("nslices", REDUCE_NSLICES)
def test_slice_sum_on_synthetic_slabs(nslices):
    E, _ = _engine()
    Cin, Cout, K = 5, 7, 3
    gen = torch.Generator().manual_seed(100 + nslices)
    d = _reduce_desc(Cin, Cout, K, 1, nslices)
    sbuf, slabs, live = _slabs(d, Cin, Cout, K, nslices, gen)
    sum64, mag = live.double().sum(0), live.double().abs().sum(0)
    for name, n, off, so, sc, taps in _layouts(Cin, Cout, K):
        idx = _dst_index(Cin, Cout, K, off, so, sc, taps)
        assert idx.unique().numel() == idx.numel() and int(idx.max()) < n
        for accumulate in (0, 1):
            what = f"slice sum nslices {nslices} {name} accumulate {accumulate}"
            prior = torch.randn(n, generator=gen)
            dbuf, dst = _guarded(n)
            if accumulate:
                dst.copy_(prior)
            before = dst.cpu().clone()
            E.check(E.lib().c2s_wgrad_reduce(ctypes.byref(d), slabs.data_ptr(), dst.data_ptr() + 4 * off, so, sc,
                                             E._tap_array(taps), accumulate, E._stream()), "wgrad_reduce")
            torch.cuda.synchronize()
            _assert_guards(what, dbuf, n)
            after = dst.cpu()
            untouched = torch.ones(n, dtype=torch.bool)
            untouched[idx.flatten()] = False
            assert torch.equal(_bits(after[untouched]), _bits(before[untouched])), f"{what}: wrote outside its elements"
            got = after[idx].double()
            assert bool(torch.isfinite(got).all()), f"{what}: read a padded channel row or column"
            p = prior[idx].double() if accumulate else torch.zeros_like(got)
            err = (got - (sum64 + p)).abs()
            bound = nslices * R.U * (mag + p.abs())
            assert bool((err <= bound).all()), f"{what}: worst |err| / (u * sum |slab|) = {float((err / (R.U * (mag + p.abs()))).max()):.2f}"
    _assert_guards(f"slice sum nslices {nslices}: slabs", sbuf, slabs.numel())


def test_batched_slice_sum_is_the_per_job_one():
    """Three jobs of different slice counts and shapes in one c2s_wgrad_reduce_batch launch: bit-identical to
    c2s_wgrad_reduce job by job.  Blocks per job: 5, 34 and 53 (the elements of none fill their last block)."""
    E, _ = _engine()
    jobs = [(5, 7, 3, 1, 5, 0), (33, 65, 1, 1, 17, 1), (3, 70, 4, 2, 2, 0)]          # Cin, Cout, K, S, nslices, accumulate
    gen = torch.Generator().manual_seed(5)
    rec = E.lib().c2s_wgrad_reduce_job_bytes()
    table = torch.zeros(len(jobs) * rec, dtype=torch.uint8).pin_memory()
    keepalive, single, batched, block, blocks = [], [], [], 0, []
    for i, (Cin, Cout, K, S, nslices, accumulate) in enumerate(jobs):
        d = _reduce_desc(Cin, Cout, K, S, nslices)
        sbuf, slabs, _ = _slabs(d, Cin, Cout, K, nslices, gen)
        n, KK = Cout * Cin * K * K, K * K
        prior = torch.randn(n, generator=gen)
        taps = E._tap_array(list(range(KK)))
        pair = []
        for _ in range(2):
            dbuf, dst = _guarded(n)
            dst.copy_(prior)
            pair.append((dbuf, dst))
        E.check(E.lib().c2s_wgrad_reduce(ctypes.byref(d), slabs.data_ptr(), pair[0][1].data_ptr(), Cin * KK, KK, taps,
                                         accumulate, E._stream()), "wgrad_reduce")
        E.check(E.lib().c2s_wgrad_reduce_job_fill(table.data_ptr() + i * rec, ctypes.byref(d), slabs.data_ptr(),
                                                  pair[1][1].data_ptr(), Cin * KK, KK, taps, accumulate, block),
                "wgrad_reduce_job_fill")
        nb = E.lib().c2s_wgrad_reduce_job_blocks(ctypes.byref(d))
        assert nb == -(-4 * n // 256)
        blocks.append(nb)
        block += nb
        single.append(pair[0][0])
        batched.append(pair[1][0])
        keepalive.append((sbuf, taps))
    assert blocks == [5, 34, 53]
    dev_table = table.cuda()
    E.check(E.lib().c2s_wgrad_reduce_batch(dev_table.data_ptr(), len(jobs), block, E._stream()), "wgrad_reduce_batch")
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(single, batched)):
        assert bool(torch.isfinite(a).all()), f"job {i}: the per-job sum read a padded channel row or column"
        assert torch.equal(_bits(a), _bits(b)), f"job {i}: the batched sum differs from the per-job sum"
        _assert_guards(f"job {i}", b, b.numel() - 2 * GUARD)


# =================================================================================================
# coverage: the instantiations the table reached
# =================================================================================================
def test_reached_instantiations_are_the_table():
    """The (family, K) pairs the rows reached are the fifteen instantiations of c2s_conv_wgrad.  Rows not run yet in this
    session (-k selections) run here."""
    for row in G.ROWS:
        if row.id not in REACHED:
            _run_row(row)
    print("\nworst |err| / (u * A) per class: " + "  ".join(f"{k} {v:.2f}" for k, v in sorted(OBSERVED.items())))
    reached = set(REACHED.values())
    assert reached == G.INSTANTIATIONS, f"missing {sorted(G.INSTANTIATIONS - reached)}, unexpected {sorted(reached - G.INSTANTIATIONS)}"
    assert {f for f, _ in reached} == set(range(7))
