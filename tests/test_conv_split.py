"""The tile-split rule of c2s_conv_igemm as a pure host query (no GPU): c2s_conv_igemm_split with cus = 256.

The split divides the positions of a tile, not the K loop (a K split rounds differently at every split, which the suite's
bit-for-bit batch-independence tests forbid: DESIGN 8), so the rule has no minimum of input channels, and c2s_conv_xpair
has no split and no query."""
import ctypes

import pytest

CUS = 256


def _lib():
    from crop2seg_amd import _lib as L
    return L


def conv_desc(N, cin, cout, H, W, K=3, S=1, c1=0):
    L = _lib()
    pad = {1: 0, 2: 0, 3: 1, 4: 1, 6: 2}[K]
    Ho, Wo = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    return L.ConvDesc(N, cin, c1, H, W, cout, (cout + 31) // 32 * 32, Ho, Wo, Ho, Wo, K, K, S, pad, pad, L.PAD_REFLECT if pad else L.PAD_ZEROS,
                      1, 1, 0, 0, 0, 0)


def igemm_split(d, cus=CUS):
    return _lib().lib().c2s_conv_igemm_split(ctypes.byref(d), cus)


def wgs1(d, frags):
    """Workgroups of the unsplit launch: fragments of 32 positions (FC = 2^l2 columns x 32 / FC rows), `frags` per tile."""
    l2 = 5
    while l2 > 2 and (1 << l2) > d.Wout:
        l2 -= 1
    FC, FR = 1 << l2, 32 >> l2
    return -(-d.Wout // FC) * -(-d.Hout // (frags * FR)) * d.N * (d.CoutP // 32)


LAYERS = [(cin, cout, hw, K, S) for cin, cout in ((32, 32), (96, 32), (64, 64), (128, 128), (32, 15), (256, 128))
          for hw in (4, 16, 32, 64, 128) for K, S in ((3, 1), (1, 1), (4, 2), (2, 1), (6, 2), (2, 2))]


def test_dominant_layer_is_not_split():
    assert igemm_split(conv_desc(128, 64, 64, 128, 128)) == 1


def test_launches_that_fill_the_gpu_are_not_split():
    n = 0
    for cin, cout, hw, K, S in LAYERS:
        for N in (1, 4, 16, 128):
            d = conv_desc(N, cin, cout, hw, hw, K, S)
            if wgs1(d, 8) >= 2 * CUS:
                n += 1
                assert igemm_split(d) == 1, (N, cin, cout, hw, K, S)
    assert n > 100


def test_split_never_decreases_as_frames_shrink():
    some = set()
    for cin, cout, hw, K, S in LAYERS:
        prev = 1
        for N in range(128, 0, -1):
            sp = igemm_split(conv_desc(N, cin, cout, hw, hw, K, S))
            assert sp in (1, 2, 4) and sp >= prev, (N, cin, cout, hw, K, S, sp, prev)
            prev = sp
        some.add(prev)
    assert some <= {1, 2, 4} and 4 in some, some        # the split each layer ends at, N = 1


def test_decoder_layers_are_split():
    # the 32-channel decoder layers of the flagship step at N = batch = 4 frames
    assert igemm_split(conv_desc(4, 96, 32, 64, 64)) == 4            # 64 workgroups unsplit
    assert igemm_split(conv_desc(4, 32, 32, 128, 128)) == 2          # 256 unsplit, 512 at split 2


def test_channel_count_does_not_enter_the_rule():
    """The split divides positions: a layer's input channels (the length of its K loop) do not enter the rule.  Measured
    (profiles/igemm_split_sweep.txt): a 1x1 layer of 16 channels, one chunk of 8 k-steps and the shortest K loop the kernel
    has, runs 10.5 us unsplit and 6.2 us at split 4, so there is no layer too small to split and no minimum to return 1 for."""
    for cin in (1, 4, 16, 64, 256):
        assert igemm_split(conv_desc(4, cin, 32, 64, 64, 1, 1)) == 4
        assert igemm_split(conv_desc(4, cin, 32, 128, 128)) == 2
        assert igemm_split(conv_desc(128, cin, 32, 128, 128)) == 1


def test_cus_argument():
    d = conv_desc(4, 32, 32, 128, 128)                                # 256 workgroups unsplit
    assert igemm_split(d, 128) == 1 and igemm_split(d, 256) == 2 and igemm_split(d, 1024) == 4
    assert igemm_split(d, 0) in (1, 2, 4) and igemm_split(d, -1) == igemm_split(d, 0)     # the current device's, 256 without one


def test_abi_version_unchanged():
    assert _lib().lib().c2s_abi_version() == 4
