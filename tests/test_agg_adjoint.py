"""CPU companion of tests/test_agg_adjoint_gpu.py: the float64 reference of norm_ref.agg_ref evaluated in float32 stays at
|err| <= 1 * u * A on every row of tests/agg_adjoint_rows.py, so the constant C_BOUND = 2 the GPU test holds the kernels to
is, for these inputs too, that plus a margin and fitted to no kernel (as test_norm_reference.py shows for norm_ref.agg_rows)."""
import pytest
import torch

import agg_adjoint_rows
import norm_ref as R
from norm_ref import bound_ratio


@pytest.mark.parametrize("row", agg_adjoint_rows.rows(), ids=lambda r: r["name"])
def test_fp32_evaluation_of_agg_adjoint_rows_stays_within_one(row):
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    assert all(bool(torch.isfinite(v).all()) for v in list(o.values()) + list(A.values())), "a padded frame leaked"
    o32 = R.agg_row_ref(row, t, dtype=torch.float32)[0]
    r = {k: bound_ratio(o32[k], o[k], A[k]) for k in A}
    assert set(r) == {"out", "gx", "gattn"} and max(r.values()) <= 1.0, {k: round(v, 3) for k, v in r.items()}
