"""Independent float64 references of the convolutions and a per-element error bound (CPU only).

The references use plain torch.nn.functional in float64 (reflect layers: F.pad(mode="reflect") and then conv2d) and
autograd for the gradients; they do not go through oracle/crop2seg_oracle.py.

Per-element bound: for a linear map y = L(x, w) the rounding error of any fp32 summation order is bounded by a small
multiple of u * L(|x|, |w|), u = 2^-24.  So the same map is evaluated on absolute values in float64:

    forward           A = conv(|x|, |w|) + |b|
    data gradient     A = vjp of conv(., |w|) at |gout|   (autograd through the reflect pad carries the adjoint fold)
    weight gradient   A = wgrad(|x|, |gout|)
    accumulation      A += |prior|

and a kernel result must satisfy |got - ref64| <= c * u * A + 1e-30 element by element.  An indexing, tiling or
accumulation bug shows up as a ratio of order 1/u ~ 1e7; the constants c of the kernel families stay far below that.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FROB_FWD = 2e-6          # the bars of tests/test_ops_gpu.py: the new checks are never looser than those
FROB_GRAD = 5e-6


def _conv(x, w, stride, pad, mode, groups, transpose):
    if transpose:
        return F.conv_transpose2d(x, w, None, stride=stride, padding=pad)
    if pad and mode == "reflect":
        return F.conv2d(F.pad(x, (pad, pad, pad, pad), mode="reflect"), w, None, stride=stride, groups=groups)
    return F.conv2d(x, w, None, stride=stride, padding=pad, groups=groups)


def conv_refs(x, w, b, gout, stride, pad, mode, groups=1, transpose=False, weight_grad=True):
    """float64 forward output, data gradient and weight gradient of the convolution at (x, w, b, gout), and their bounds
    A (same map on absolute values).  All tensors on the CPU, real frames only.  weight_grad=False leaves "gw" / "Agw" None
    (a third of the work, for callers that check the forward and the data gradient of many frames)."""
    def run(xs, ws, bs, gs):
        xs = xs.detach().double().requires_grad_(True)
        ws = ws.detach().double().requires_grad_(weight_grad)
        y = _conv(xs, ws, stride, pad, mode, groups, transpose)
        if bs is not None:
            y = y + bs.detach().double().view(1, -1, 1, 1)
        y.backward(gs.detach().double())
        return y.detach(), xs.grad, ws.grad

    y, gx, gw = run(x, w, b, gout)
    ay, agx, agw = run(x.abs(), w.abs(), None if b is None else b.abs(), gout.abs())
    return {"y": y, "gx": gx, "gw": gw, "Ay": ay, "Agx": agx, "Agw": agw}


def bound_ratio(got, ref, A):
    """max |got - ref| / (u * A): the smallest c for which the per-element bound holds."""
    err = (got.detach().double().cpu() - ref).abs()
    return float((err / (U * A + 1e-30)).max())


def assert_within(what, got, ref, A, c, frob):
    """All finite, the Frobenius relative error below `frob`, and |got - ref| <= c * u * A + 1e-30 element by element.
    Returns the observed ratio max |got - ref| / (u * A)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
    fr = float((got - ref).norm() / (ref.norm() + 1e-30))
    assert fr < frob, f"{what}: Frobenius relative error {fr:.3e} >= {frob:.1e}"
    err = (got - ref).abs()
    bad = err > c * U * A + 1e-30
    if bool(bad.any()):
        i = int(torch.argmax((err / (U * A + 1e-30)).flatten()))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        c_at = float(torch.broadcast_to(torch.as_tensor(c, dtype=torch.float64), got.shape)[idx])
        raise AssertionError(f"{what}: {int(bad.sum())} elements beyond c * u * A; worst at {idx} (c = {c_at:g}): "
                             f"got {got[idx]:.9e}, ref {ref[idx]:.9e}, |err| / (u * A) = {float(err[idx] / (U * A[idx] + 1e-30)):.3e}")
    return float((err / (U * A + 1e-30)).max())


def check_conv(got_y, got_gx, got_gw, x, w, b, gout, keep, stride, pad, mode, c, prior=None, sentinel=None, groups=1,
               transpose=False):
    """Check one convolution's kernel results against the float64 references.

    got_y / got_gx / got_gw: full-batch kernel outputs (got_gx may be None when no data gradient ran); x / gout: the full
    batch (padded frames may hold anything, NaN included); keep: bool per frame (real frames); prior: the gradient that was
    on x before the backward pass (None: none; zeros where a source had none); sentinel: bool mask over got_gx of the
    elements that must still be bit-identical to `prior` (the padded frames of an accumulated gradient).  c: dict with the
    constants "fwd", "dgrad", "wgrad".  Returns the observed ratios {"fwd", "dgrad", "wgrad"}."""
    R = conv_refs(x[keep], w, b, gout[keep], stride, pad, mode, groups, transpose)
    ratios = {"fwd": assert_within("forward", got_y[keep], R["y"], R["Ay"], c["fwd"], FROB_FWD)}
    if got_gx is not None:
        ref, A = R["gx"], R["Agx"]
        if prior is not None:
            p = prior[keep].double()
            ref, A = ref + p, A + p.abs()
        ratios["dgrad"] = assert_within("data gradient", got_gx[keep], ref, A, c["dgrad"], FROB_GRAD)
        if sentinel is not None and bool(sentinel.any()):
            same = got_gx.cpu()[sentinel].view(torch.int32) == prior[sentinel].view(torch.int32)
            assert bool(same.all()), f"padded-frame gradient overwritten: {int((~same).sum())} of {int(sentinel.sum())} elements"
    assert bool(torch.isfinite(got_gw.cpu()).all()), "weight gradient not finite (a kernel read a padded frame?)"
    ratios["wgrad"] = assert_within("weight gradient", got_gw, R["gw"], R["Agw"], c["wgrad"], FROB_GRAD)
    return ratios
