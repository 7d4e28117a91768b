"""Rows for the adjoint of the attention upsampling (agg_upsample_adjoint_kernel of csrc/aggregate.hip), in the format of
norm_ref.agg_rows(): shared by tests/test_agg_adjoint.py (CPU) and tests/test_agg_adjoint_gpu.py.

The kernel walks the rows of a plane once per column, keeps the running sums of two low-resolution rows and parks
finished ones in LDS; a plane whose parked rows exceed 8192 floats is cut into tiles.  The rows cover every ratio the
walk treats differently (8, 4, 2, 1 and mixed), columns beyond one workgroup, a width that is no multiple of a wave, a
single attention row (nothing is ever parked before the end), and one plane large enough to be cut in both directions
(h (W + 1) = 16 * 2049 > 8192 and more than 1024 columns: tiles of 8 x 64 cells with their halos)."""


def rows():
    R = lambda name, B, T, C, nh, H, W, h, w, **kw: dict(name=name, B=B, T=T, C=C, nh=nh, H=H, W=W, h=h, w=w, **kw)   # noqa: E731
    return [R("ratio8", 1, 2, 16, 16, 32, 128, 4, 16),
            R("ratio4", 1, 2, 16, 16, 16, 64, 4, 16),
            R("ratio2", 1, 2, 16, 16, 8, 32, 4, 16),
            R("mixed_2x8", 1, 2, 16, 16, 8, 64, 4, 8),
            R("w_beyond_a_workgroup", 1, 2, 16, 16, 4, 512, 2, 64),
            R("w_not_a_multiple_of_64", 1, 2, 16, 16, 8, 24, 1, 3),
            R("rows_ratio1_columns_ratio4", 1, 2, 16, 16, 4, 64, 4, 16),
            R("padded_frame_prior_gattn", 2, 3, 32, 16, 16, 32, 2, 4, pad=[(1, 1)], prior_gattn=True),
            R("tiled_plane", 1, 2, 16, 16, 32, 2048, 16, 256)]
