"""The depthwise kernels (csrc/misc.hip: dw_fwd_kernel, dw_dgrad_kernel, dw_wgrad_kernel, dw_wgrad_reduce_kernel) at every edge
of their dispatch against the float64 references of tests/conv_ref.py, element by element.

The rows are those of tests/dw_ref.py (the table, its reasons and its inputs are there; test_dw_plan.py holds the same rows
against the host query and the reference against itself, without a GPU).  Conventions of test_conv_paths_gpu.py: padded
frames hold NaN in x and gout; an accumulated prior holds 1234.5 on the padded frames and must come back bit-identical;
conv_ref.check_conv(..., groups=C) applies |got - ref64| <= c * u * A per element and the Frobenius bars.  In addition a
data gradient that does not accumulate is exactly 0 on the padded frames, as the kernel writes it.  Every row asserts the
pixels per thread of its three exports (c2s_dwconv_paths, whose predicates the launchers call) against its literal, and
test_rows_reached_every_variant asserts what the rows reached together.

Constants: C_FAMILY["dw"] = 16 and C_FAMILY["dw_wgrad"] = 8 of test_conv_paths_gpu.py, C_OP = 32 of
test_strided_geometry_gpu.py for (6,2,2); none had to move.  Worst ratios max |err| / (u * A) observed on an MI355X (printed
with -s), per geometry, export and pixels per thread:

    (3,1,1)   fwd 4: 3.22   fwd 1: 2.52   dgrad 4 (stencil): 3.18   dgrad 1 (gather): 2.45   wgrad 4: 1.10   wgrad 1: 2.05
    (4,2,1)   fwd 4: 3.37   fwd 1: 1.99   dgrad 4 (stencil): 2.66   dgrad 1 (gather): 1.81   wgrad 4: 1.43   wgrad 1: 1.66
    (6,2,2)   fwd 1: 4.05                 dgrad 1 (gather): 3.06                             wgrad 1: 0.17

(k4-n130, the weight gradient over 126 real frames with three frames on two lanes of the reduction: 0.09.)

The rows can fail: against a library built from the previous misc.hip (four pair slots in the gather's list; the query
added to it unchanged; a local build that is not part of the project) exactly k3-h3, k3-w3 and k3-3x3 failed on an MI355X,
each on the data gradient alone, with Frobenius relative errors 2.6e-1, 4.0e-1 and 3.5e-1; the other rows passed with the
ratios above.  (The two k4-odd-w rows were left out of that run: the previous dispatch puts them on float4 loads of rows
that are 4-byte aligned only.)
"""
import pytest
import torch

import conv_ref as R
import dw_ref as D
from test_conv_paths_gpu import _ctx

pytestmark = pytest.mark.gpu

REACHED = {}            # row id -> (geometry, (fwd, dgrad, wgrad))
OBSERVED = {}           # (geometry, export, pixels per thread) -> worst ratio


def _engine():
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    return E, _lib


def _note(row, ratios):
    for i, k in enumerate(("fwd", "dgrad", "wgrad")):
        key = (f"k{row.K}", k, row.paths[i])
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), ratios[k])


def _run_row(row):
    E, L = _engine()
    t = D.inputs(row)
    c = D.constants(row)
    keep, w, b = t["keep"], t["w"], t["b"]
    N = row.N
    pm = L.PAD_REFLECT if row.mode == "reflect" else L.PAD_ZEROS
    triple = D.row_paths(L, row)
    assert triple == row.paths, f"{row.id}: c2s_dwconv_paths reports {triple}, the table says {row.paths}"
    ctx = _ctx({"w": w} if b is None else {"w": w, "b": b})
    vd = keep.int().cuda()
    live = []                                                   # (x, out, gout) on the device: the tape keys by data_ptr
    for x, gout, prior in t["calls"]:
        xd = x.cuda()
        if prior is not None:
            ctx.tape.grads[xd.data_ptr()] = prior.cuda()
        out = E.depthwise_conv2d(ctx, xd, "w", row.K, row.S, row.pad, pm, vd, bname=None if b is None else "b")
        assert tuple(out.shape) == (N, D.C) + D.out_hw(row)
        live.append((xd, out, gout.cuda()))
    for _, out, gd in live:                                     # seed every output, then one backward pass
        ctx.tape.grads[out.data_ptr()] = gd
    ctx.tape.backward()
    torch.cuda.synchronize()
    got_gw = ctx.g["w"].cpu()
    sentinel = (~keep).view(N, 1, 1, 1).expand(N, D.C, row.H, row.W).clone()
    ratios = {"fwd": 0.0, "dgrad": 0.0, "wgrad": 0.0}
    if row.kind != "twice":
        (x, gout, prior), (xd, out, _) = t["calls"][0], live[0]
        got_gx = ctx.tape.grads[xd.data_ptr()].cpu()
        ratios = R.check_conv(out.cpu(), got_gx, got_gw, x, w, b, gout, keep, row.S, row.pad, row.mode, c, prior=prior,
                              sentinel=sentinel if prior is not None else None, groups=D.C)
        if prior is None:
            assert bool((got_gx[~keep] == 0).all()), f"{row.id}: a fresh data gradient is not 0 on the padded frames"
    else:
        # the weight gradient against the sum of the two float64 references, A summed likewise
        gw, Agw = 0, 0
        for (x, gout, prior), (xd, out, _) in zip(t["calls"], live):
            r = D.refs(row, x, w, b, gout, prior, keep)
            got_gx = ctx.tape.grads[xd.data_ptr()].cpu()
            ratios["fwd"] = max(ratios["fwd"], R.assert_within("forward", out.cpu()[keep], r["y"], r["Ay"], c["fwd"], R.FROB_FWD))
            ratios["dgrad"] = max(ratios["dgrad"], R.assert_within("data gradient", got_gx[keep], r["gx"], r["Agx"], c["dgrad"],
                                                                   R.FROB_GRAD))
            assert bool((got_gx[~keep] == 0).all()), f"{row.id}: a fresh data gradient is not 0 on the padded frames"
            gw, Agw = gw + r["gw"], Agw + r["Agw"]
        ratios["wgrad"] = R.assert_within("weight gradient written twice", got_gw, gw, Agw, c["wgrad"], R.FROB_GRAD)
    REACHED[row.id] = ((row.K, row.S, row.pad), triple)
    _note(row, ratios)
    print(f"\n{row.id}: {triple} " + "  ".join(f"{k} {v:.2f}" for k, v in ratios.items()))


@pytest.mark.parametrize("row", D.ROWS, ids=D.IDS)
def test_depthwise_row(row):
    _run_row(row)


def test_rows_reached_every_variant():
    """For (3,1,1) and (4,2,1): both variants of the forward, the data gradient and the weight gradient, and the triples on
    which the forward and the data gradient differ.  Rows not run yet in this session (-k selections) run here."""
    for row in D.ROWS:
        if row.id not in REACHED:
            _run_row(row)
    print("\nworst |err| / (u * A): " + "  ".join(f"{g}/{k}/{px} {v:.2f}" for (g, k, px), v in sorted(OBSERVED.items())))
    for geom in D.REACHED_BOTH:
        triples = {tr for g, tr in REACHED.values() if g == geom}
        for i, k in enumerate(("fwd", "dgrad", "wgrad")):
            assert {tr[i] for tr in triples} == {1, 4}, f"{geom}: {k} reached {sorted({tr[i] for tr in triples})} pixels per thread"
        assert D.MIXED[geom] <= triples, f"{geom}: mixed triples missing: {sorted(D.MIXED[geom] - triples)}"
    assert {tr for g, tr in REACHED.values() if g == (6, 2, 2)} == {(1, 1, 1)}
