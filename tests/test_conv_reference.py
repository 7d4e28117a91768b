"""The fp64 reference checker of tests/conv_ref.py must be able to fail (CPU only).

A CPU fp32 torch convolution plays the kernel: unchanged it passes the per-element bound; each mutation that a broken
accumulate / reflect-adjoint / padded-frame path of a HIP kernel would produce must be rejected."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

N, CIN, COUT, H, W = 3, 8, 12, 10, 14       # 10 x 14: partial 4 x 4 / 2 x 2 tiles in both directions
SENTINEL = 1234.5
C_CPU = {"fwd": 16, "dgrad": 16, "wgrad": 16}


def _case():
    g = torch.Generator().manual_seed(3)
    keep = torch.tensor([True, False, True])
    x = torch.randn(N, CIN, H, W, generator=g)
    x[~keep] = float("nan")
    w = torch.randn(COUT, CIN, 3, 3, generator=g) / 8
    b = torch.randn(COUT, generator=g)
    gout = torch.randn(N, COUT, H, W, generator=g)
    gout[~keep] = float("nan")
    prior = torch.randn(N, CIN, H, W, generator=g)
    prior[~keep] = SENTINEL
    sentinel = (~keep).view(N, 1, 1, 1).expand(N, CIN, H, W).clone()
    return x, w, b, gout, keep, prior, sentinel


def _fp32_kernel(x, w, b, gout, keep, prior, mode="reflect"):
    """fp32 CPU convolution over the real frames: full-batch outputs as an accumulating kernel leaves them (padded frames
    of the data gradient untouched)."""
    xs = x[keep].clone().requires_grad_(True)
    ws = w.clone().requires_grad_(True)
    xp = F.pad(xs, (1, 1, 1, 1), mode="reflect") if mode == "reflect" else F.pad(xs, (1, 1, 1, 1))
    y = F.conv2d(xp, ws, b)
    y.backward(gout[keep])
    got_y = torch.full((N, COUT, H, W), float("nan"))
    got_y[keep] = y.detach()
    got_gx = prior.clone()
    got_gx[keep] += xs.grad
    return got_y, got_gx, ws.grad


def _check(got_y, got_gx, got_gw, case):
    x, w, b, gout, keep, prior, sentinel = case
    return R.check_conv(got_y, got_gx, got_gw, x, w, b, gout, keep, 1, 1, "reflect", C_CPU, prior=prior, sentinel=sentinel)


def test_unmutated_fp32_convolution_passes():
    case = _case()
    ratios = _check(*_fp32_kernel(*case[:6]), case)
    assert all(0 < r < C_CPU[k] for k, r in ratios.items()), ratios


def _mut_no_reflect_fold(y, gx, gw, case):
    x, w, b, gout, keep, prior, _ = case
    _, gz, _ = _fp32_kernel(x, w, b, gout, keep, prior, mode="zeros")
    gx[:, :, 1, :] = gz[:, :, 1, :]                         # row 1 misses the fold of padded row -1
    return y, gx, gw


def _mut_prior_dropped(y, gx, gw, case):
    keep, prior = case[4], case[5]
    gx[keep] -= prior[keep]
    return y, gx, gw


def _mut_prior_twice(y, gx, gw, case):
    keep, prior = case[4], case[5]
    gx[keep] += prior[keep]
    return y, gx, gw


def _mut_partial_tile_pixel(y, gx, gw, case):
    x, w, b, gout, keep = case[:5]
    A = R.conv_refs(x[keep], w, b, gout[keep], 1, 1, "reflect")["Ay"]
    y[2, 5, H - 1, W - 1] += 1e3 * R.U * float(A[1, 5, H - 1, W - 1])   # last pixel of the last (partial) tile of frame 2
    return y, gx, gw


def _mut_sentinel(y, gx, gw, case):
    gx[1, 3, 4, 5] = 0.0                                       # a write into the padded frame
    return y, gx, gw


@pytest.mark.parametrize("mutate", [_mut_no_reflect_fold, _mut_prior_dropped, _mut_prior_twice, _mut_partial_tile_pixel,
                                    _mut_sentinel], ids=lambda f: f.__name__[5:])
def test_mutation_is_rejected(mutate):
    case = _case()
    got = mutate(*_fp32_kernel(*case[:6]), case)
    with pytest.raises(AssertionError):
        _check(*got, case)

