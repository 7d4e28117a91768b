"""The adjoint of the attention upsampling (agg_upsample_adjoint_kernel of csrc/aggregate.hip) through the backward of
engine.temporal_aggregate, element by element against the float64 reference of tests/norm_ref.py at the project's bounds
(|got - ref| <= C_BOUND u A next to FROB["gattn"]), on the rows of tests/agg_adjoint_rows.py: every ratio between feature
map and attention map the row walk treats differently, planes wider than a workgroup, narrower than a wave and large enough
to be cut into tiles.  tests/test_agg_adjoint.py shows on the CPU that a float32 evaluation of the reference stays within 1
on these rows.  Then: two runs give equal bits, and a sample's gradient does not depend on the batch it is in."""
import pytest
import torch

import agg_adjoint_rows
import norm_ref as R
from norm_ref import assert_within

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def backward(t, nh, mode="att_group"):
    """engine.temporal_aggregate and its backward on the tensors of norm_ref.agg_inputs; returns (gx, gattn) on the CPU."""
    from crop2seg_amd import engine as E
    dev = torch.device("cuda")
    ctx = E.Ctx({}, {}, {}, E.Workspace(dev), True, E.Tape())
    x5, ad = t["x"].cuda(), t["attn"].cuda()
    keep = t["valid"]
    vd = keep.view(-1).int().cuda() if not bool(keep.all()) else None
    out = E.temporal_aggregate(ctx, x5, ad, vd, nh, mode)
    if t["prior_gattn"] is not None:
        ctx.tape.grads[ad.data_ptr()] = t["prior_gattn"].cuda().clone()
    ctx.tape.grads[out.data_ptr()] = t["gout"].cuda().clone()
    ctx.tape.backward()
    torch.cuda.synchronize()
    return ctx.tape.grads[x5.data_ptr()].cpu(), ctx.tape.grads[ad.data_ptr()].cpu()


@pytest.mark.parametrize("name", [r["name"] for r in agg_adjoint_rows.rows()])
def test_agg_adjoint_rows_per_element(name):
    row = next(r for r in agg_adjoint_rows.rows() if r["name"] == name)
    t = R.agg_inputs(row)
    o, A = R.agg_row_ref(row, t)
    gx, ga = backward(t, row["nh"])
    keep = t["valid"]
    pad = ~keep
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(ga).all()), "non-finite values (a padded frame was read?)"
    r = assert_within(f"{name} gattn", ga[:, keep], o["gattn"][:, keep], A["gattn"][:, keep], R.C_BOUND, R.FROB["gattn"])
    rx = assert_within(f"{name} gx", gx[keep], o["gx"][keep], A["gx"][keep], R.C_BOUND, R.FROB["agg_gx"])
    print(f"{name}: |err| / (u A)  gattn {r:.3f}  gx {rx:.3f}")
    if bool(pad.any()):
        assert t["prior_gattn"] is not None
        assert same_bits(ga[:, pad], t["prior_gattn"][:, pad]), "the gradient already on a padded frame was touched"
        assert bool((bits(gx[pad]) == 0).all()), "gradient of a padded frame is not 0"


@pytest.mark.parametrize("name", ["ratio8", "padded_frame_prior_gattn", "tiled_plane"])
def test_two_runs_give_equal_bits(name):
    row = next(r for r in agg_adjoint_rows.rows() if r["name"] == name)
    t = R.agg_inputs(row)
    a, b = backward(t, row["nh"]), backward(t, row["nh"])
    assert same_bits(a[1], b[1]) and same_bits(a[0], b[0])


def test_a_sample_alone_and_in_a_batch_of_three_gives_equal_bits():
    row = dict(name="b3", B=3, T=2, C=16, nh=16, H=32, W=128, h=4, w=16)
    t = R.agg_inputs(row)
    alone = dict(x=t["x"][:1].contiguous(), attn=t["attn"][:, :1].contiguous(), gout=t["gout"][:1].contiguous(),
                 valid=t["valid"][:1], prior_gx=None, prior_gattn=None)
    ga3 = backward(t, row["nh"])[1]
    ga1 = backward(alone, row["nh"])[1]
    assert same_bits(ga3[:, :1], ga1)
