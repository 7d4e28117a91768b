"""Independent float64 references of the activation-sized kernels next to the convolutions and the L-TAE, each with a
per-element error bound (CPU only): GroupNorm / BatchNorm (+ReLU, +residual) of csrc/norm.hip, squeeze-and-excitation of
csrc/se.hip, the temporal aggregation of csrc/aggregate.hip and the dropout + per-pixel GroupNorm pair of the L-TAE MLP.

Every reference is written out as explicit formulas (forward and backward, no autograd, no F.group_norm / F.batch_norm /
F.interpolate; tests/test_norm_reference.py ties them to those), each line next to its bound.  A reference returns
({name: value}, {name: A}) for the real frames, like ltae_ref.ltae_ref, and a kernel result must satisfy

    |got - ref64| <= C_BOUND * u * A + 1e-30,     u = 2^-24,     C_BOUND = 2 for every output,

element by element (conv_ref.assert_within), next to the Frobenius bars of tests/test_ops_gpu.py.

A is first-order propagation of per-operation rounding, so a correct fp32 evaluation has a ratio |err| / (u A) of at most
1 plus second-order terms, in any order of evaluation; C_BOUND = 2 is that plus a margin and is NOT fitted to the kernels: it
is calibrated against the references alone -- the same formulas evaluated with dtype=torch.float32 (torch's own summation
order) must stay <= 1 on every row of the GPU tables (test_norm_reference.py::test_fp32_evaluation_*).  A kernel that
legitimately needs more gets a named term in A, never a larger constant.  Such terms so far:

    RSQRT_ULPS  accuracy of rsqrtf (eval-mode BatchNorm, per-pixel GroupNorm), in ulp of its result
    EXP_ULPS    accuracy of expf in the sigmoid of squeeze-and-excitation, in ulp of its result

Both start at 2 ulp (nobody had measured them for this project).  MI355X run of tests/test_norm_reference_gpu.py: the worst
ratios where they enter were 0.70 (y over the two-pass BatchNorm rows, eval mode among them), 0.42 (y of the per-pixel
GroupNorm) and 0.66 (y of squeeze-and-excitation), so 2 ulp each was never the binding term and neither allowance grew; the full table is in that
file's docstring.

Normalisation (linear steps carry the same map on absolute values, as in conv_ref.py; this is the bound derived in
tests/ltae_ref.py, regrouped over (channels of the group x HW) for GroupNorm and (valid frames x HW) for BatchNorm):

    m = mean(x)                     A_m   = mean|x|
    d = x - m;  var = mean(d^2)     A_var = var + 2 mean(|d| (|x| + |m|))
    r = 1 / sqrt(var + eps)         A_r   = r A_var / (2 (var + eps)) + r (1.5 + 2 RSQRT_ULPS)
    xhat = d r                      A_xh  = r (A_m + |x| + |m|) + |d| A_r
    pre = gamma xhat + beta         A_pre = |gamma| (A_xh + |xhat|) + |beta|
    y = relu(pre) (+ res)           A_y   = A_pre (+ |y| + |res|)
    g' = g [pre > 0];  gxh = gamma g'
    m1 = mean(gxh); m2 = mean(gxh xhat)      A_m1 = mean|gxh|,  A_m2 = mean(2 |gxh xhat| + |gxh| A_xh)
    gx = r (gxh - m1 - xhat m2)     A_gx  = A_r |inner| + r (2 |gxh| + A_m1 + |m1| + |xhat| (A_m2 + |m2|) + A_xh |m2|)

A_xh grows linearly with |m| / sigma (a rounded mean and a folded shift x r - m r are legitimate kernel forms); a variance
of the form E[x^2] - E[x]^2 errs by u (m / sigma)^2 and fails the offset cases.  Statistics that are constants (eval-mode
BatchNorm) have A_m = A_var = 0.  A sum of n terms rounds its partial sums too (log2 n times in a pairwise or lane-split
order, each by at most u |partial|): the parameter sums carry 2 sum|terms|.  For the parameter sums A adds |terms| while the sums cancel, so there the Frobenius bar is
the sharper check of a lost partial and the bound catches a wrong channel row.

ReLU kink: a gate that flips between fp32 and fp64 changes a whole group's sums and cannot be excused per element, so no
element is left out: the input builders below move the offending inputs until |pre-activation| > KINK u A_pre holds for
every element in the float64 view of the fp32 inputs, and assert that this took at most 8 rounds.

Nothing here imports crop2seg_amd or oracle.
"""
import math

import torch

from conv_ref import U, assert_within, bound_ratio  # noqa: F401  (re-exported: the tests take them from here)

C_BOUND = 2.0
RSQRT_ULPS = 2.0
EXP_ULPS = 2.0
KINK = 64.0
# the bars of tests/test_ops_gpu.py (never looser than those)
FROB = {"y": 2e-6, "gx": 2e-5, "dgamma": 2e-5, "dbeta": 2e-5, "dbias": 1e-4, "g_residual": 1e-6, "running_mean": 1e-5,
        "running_var": 1e-5, "group_stats": 1e-5,
        "se_y": 2e-6, "se_gx": 5e-6, "gW1": 2e-5, "gW2": 2e-5,
        "out": 2e-6, "agg_gx": 2e-6, "gattn": 1e-5,
        "pgn_y": 2e-6, "pgn_gx": 2e-5}


def _f(t, dtype):
    return None if t is None else t.detach().to(dtype).cpu()


# ------------------------------------------------------------------------------------------------ normalisation
def _norm_core(x, gam, bet, dims, psum, eps, relu, res, g, fixed, variance, rsqrt_ulps, A_in, bounds):
    """The formulas of the module docstring on x of any shape: statistics over `dims` (keepdim), parameter sums over `psum`;
    gam / bet broadcast against x.  fixed = (m, var): constant statistics.  A_in: bound already on x (an upstream op)."""
    mean = lambda t: t.mean(dims, keepdim=True)      # noqa: E731
    if fixed is not None:
        m, var = fixed
        d = x - m
    else:
        m = mean(x)
        d = x - m
        var = (mean(x * x) - m * m).clamp_min(0) if variance == "naive" else mean(d * d)
    r = 1.0 / torch.sqrt(var + eps)
    xh = d * r
    pre = xh * gam + bet
    act = pre.clamp_min(0) if relu else pre
    y = act if res is None else act + res
    o = {"y": y, "pre": pre, "m": m, "var": var, "r": r}
    A = {}
    if g is not None:
        gp = g * (pre > 0).to(g.dtype) if relu else g
        gxh = gp * gam
        if fixed is None:
            m1, m2 = mean(gxh), mean(gxh * xh)
        else:
            m1 = m2 = torch.zeros_like(m)
        inner = gxh - m1 - xh * m2
        gx = r * inner
        o.update(gx=gx, dgamma=(gp * xh).sum(psum), dbeta=gp.sum(psum), dbias=gx.sum(psum))
    if not bounds:
        return o, A
    X = x.abs() if A_in is None else x.abs() + A_in
    if fixed is None:
        A_m = mean(X)
        A_var = var + 2 * mean(d.abs() * (X + m.abs()))
    else:
        A_m = A_var = torch.zeros_like(m)
    A_r = r * A_var / (2 * (var + eps)) + r * (1.5 + 2 * rsqrt_ulps)
    A_xh = r * (A_m + X + m.abs()) + d.abs() * A_r
    A_pre = gam.abs() * (A_xh + xh.abs()) + bet.abs()
    A_y = A_pre if res is None else A_pre + y.abs() + res.abs()
    A.update(y=A_y, pre=A_pre, m=A_m + m.abs(), var=A_var + var, r=A_r)
    if g is not None:
        A_gxh = gxh.abs()                                       # rounding of gamma * g'
        if fixed is None:
            A_m1 = mean(A_gxh)
            A_m2 = mean(A_gxh * xh.abs() + gxh.abs() * A_xh + (gxh * xh).abs())
        else:
            A_m1 = A_m2 = torch.zeros_like(m)
        A_gx = A_r * inner.abs() + r * (A_gxh + A_m1 + xh.abs() * A_m2 + A_xh * m2.abs()
                                        + gxh.abs() + m1.abs() + (xh * m2).abs())
        A.update(gx=A_gx, dgamma=(gp.abs() * A_xh + 2 * (gp * xh).abs()).sum(psum), dbeta=2 * gp.abs().sum(psum),
                 dbias=(A_gx + gx.abs()).sum(psum))
    return o, A


def norm_ref(x, gamma, beta, kind, groups=4, training=True, running=None, residual=None, relu=True, valid=None, gout=None,
             eps=1e-5, momentum=0.1, dtype=torch.float64, variance="two_pass", bounds=True):
    """GroupNorm (kind "group": `groups` channel groups per frame) or BatchNorm2d (kind "batch": per channel over the valid
    frames; training=False: the running statistics) (+ReLU) (+residual) and its backward at gout.

    x, residual, gout [N,C,...] (padded frames may hold anything); gamma / beta [C] or None (no affine); running =
    (running_mean, running_var) [C]; valid [N] bool or None.  dtype float32: a plain fp32 evaluation of the same formulas
    (no bounds); variance="naive": E[x^2] - E[x]^2 (for the checker's own tests).

    Returns, for the real frames: y, pre (the pre-activation), gx [n,C,...]; dgamma, dbeta, dbias [C] (dbias: per-channel sum
    of gx, the gradient of the producing convolution's bias); g_residual [n,C,...]; group_stats (mean, rstd) [n,groups,2] /
    [C,2]; running_mean, running_var [C] (training BatchNorm: the updated buffers, unbiased variance)."""
    bounds = bounds and dtype == torch.float64
    keep = torch.ones(x.shape[0], dtype=torch.bool) if valid is None else valid.bool().cpu()
    xs = _f(x, dtype)[keep]
    n, C = xs.shape[:2]
    shape = xs.shape
    HW = xs[0, 0].numel()
    res = None if residual is None else _f(residual, dtype)[keep]
    g = None if gout is None else _f(gout, dtype)[keep]
    gam = torch.ones(C, dtype=dtype) if gamma is None else _f(gamma, dtype)
    bet = torch.zeros(C, dtype=dtype) if beta is None else _f(beta, dtype)
    batch = kind == "batch"
    G, cpg = (C, 1) if batch else (groups, C // groups)
    v4 = lambda t: None if t is None else t.reshape(n, G, cpg, HW)      # noqa: E731
    dims = (0, 2, 3) if batch else (2, 3)
    fixed = None
    if batch and not training:
        fixed = tuple(_f(t, dtype).view(1, C, 1, 1) for t in running)
    o, A = _norm_core(v4(xs), gam.view(1, G, cpg, 1), bet.view(1, G, cpg, 1), dims, (0, 3), eps, relu, v4(res), v4(g), fixed,
                      variance, RSQRT_ULPS if fixed is not None else 0.0, None, bounds)
    out, Aout = {}, {}
    for k in ("y", "pre", "gx"):
        if k in o:
            out[k] = o[k].reshape(shape)
            if bounds:
                Aout[k] = A[k].reshape(shape)
    for k in ("dgamma", "dbeta", "dbias"):
        if k in o:
            out[k] = o[k].reshape(C)
            if bounds:
                Aout[k] = A[k].reshape(C)
    if g is not None and res is not None:
        out["g_residual"] = g.reshape(shape)                      # the residual branch takes g itself
        if bounds:
            Aout["g_residual"] = torch.zeros(shape, dtype=torch.float64)
    m, r = o["m"].expand(1 if batch else n, G, 1, 1), o["r"].expand(1 if batch else n, G, 1, 1)
    out["group_stats"] = torch.stack([m, r], -1).reshape((C, 2) if batch else (n, G, 2))
    if bounds:
        Aout["group_stats"] = torch.stack([A["m"].expand_as(m), A["r"].expand_as(r)], -1).reshape(out["group_stats"].shape)
    if batch and training and running is not None:
        rm, rv = (_f(t, dtype) for t in running)
        cnt = n * HW
        unb = o["var"].reshape(C) * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
        mm = o["m"].reshape(C)
        out["running_mean"] = (1 - momentum) * rm + momentum * mm
        out["running_var"] = (1 - momentum) * rv + momentum * unb
        if bounds:
            Aout["running_mean"] = (1 - momentum) * rm.abs() + momentum * A["m"].reshape(C) + out["running_mean"].abs()
            Aout["running_var"] = ((1 - momentum) * rv.abs() + momentum * A["var"].reshape(C) * (cnt / (cnt - 1.0) if cnt > 1 else 1.0)
                                   + out["running_var"].abs())
    return out, Aout


def push_off_kink(x, gamma, beta, kind, groups=4, training=True, running=None, valid=None, eps=1e-5, rounds=8):
    """x (float32) with the inputs that sit on the ReLU kink moved off it: repeated until |pre| > KINK u A_pre holds for every
    element of the real frames in the float64 view of the fp32 tensor.  Returns (x, rounds used); raises when 8 rounds do not
    do it (a channel with gamma = 0 cannot be moved: give it a beta away from 0)."""
    x = x.clone()
    keep = torch.ones(x.shape[0], dtype=torch.bool) if valid is None else valid.bool().cpu()
    C = x.shape[1]
    gam = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    gv = gam.view(1, C, *([1] * (x.dim() - 2)))
    for it in range(rounds + 1):
        o, A = norm_ref(x, gamma, beta, kind, groups, training, running, None, True, valid, None, eps)
        bad = o["pre"].abs() <= KINK * U * A["pre"]
        if not bool(bad.any()):
            return x, it
        assert it < rounds, f"push_off_kink: {int(bad.sum())} elements still on the kink after {rounds} rounds"
        gs = o["group_stats"][..., 1]
        r = gs.view(1, C) if kind == "batch" else gs.repeat_interleave(C // groups, dim=1)
        r = r.reshape(-1, C, *([1] * (x.dim() - 2)))
        assert bool((gv.expand_as(bad)[bad] != 0).all()), "push_off_kink: gamma = 0 and beta on the kink"
        step = 4 * KINK * U * A["pre"] / (gv.abs() * r).clamp_min(1e-300)
        sgn = torch.where(o["pre"] >= 0, 1.0, -1.0) * torch.sign(gv)
        xs = x[keep].double()
        xs[bad] = (xs + sgn * step)[bad]
        x[keep] = xs.float()
    raise AssertionError("unreachable")


# ------------------------------------------------------------------------------------------------ squeeze-and-excitation
def se_ref(x, W1, W2, valid=None, gout=None, prior_w1=None, prior_w2=None, dtype=torch.float64, bounds=True):
    """y = x * sigmoid(W2 relu(W1 mean_hw(x))) per frame, W1 [C/16,C], W2 [C,C/16], and its backward at gout; prior_w1 /
    prior_w2: the gradient already on a weight (the kernels add to it).  Returns y, gx [n,C,...], gW1, gW2, z1 [n,R] (the
    pre-activation of the hidden ReLU) for the real frames.

        p = mean_hw x;  z1 = W1 p;  h = relu(z1);  z2 = W2 h       linear maps: the same map on absolute values
        s = 1 / (1 + exp(-z2))        A_s = s (1 - s) (A_z2 + 2 EXP_ULPS) + 2 s     (exp, then the sum and the division)
        y = x s                       A_y = |x| A_s + |y|
        ds = sum_hw g x;  dz2 = ds s (1 - s);  gW2 = sum_n dz2 h^T;  dh = W2^T dz2;  dz1 = dh [z1 > 0]
        gW1 = sum_n dz1 p^T;  dp = W1^T dz1;  gx = g s + dp / HW"""
    bounds = bounds and dtype == torch.float64
    keep = torch.ones(x.shape[0], dtype=torch.bool) if valid is None else valid.bool().cpu()
    xs = _f(x, dtype)[keep]
    shape = xs.shape
    n, C = shape[:2]
    xs = xs.reshape(n, C, -1)
    HW = xs.shape[-1]
    W1, W2 = _f(W1, dtype), _f(W2, dtype)
    p = xs.mean(-1)
    z1 = p @ W1.T
    h = z1.clamp_min(0)
    z2 = h @ W2.T
    s = 1.0 / (1.0 + torch.exp(-z2))
    y = xs * s[..., None]
    out, A = {"y": y.reshape(shape), "z1": z1}, {}
    if bounds:
        aW1, aW2 = W1.abs(), W2.abs()
        A_p = xs.abs().mean(-1) + p.abs()
        A_z1 = (A_p + p.abs()) @ aW1.T
        A_z2 = (A_z1 + h.abs()) @ aW2.T
        A_s = s * (1 - s) * (A_z2 + 2 * EXP_ULPS) + 2 * s
        A["y"] = (xs.abs() * A_s[..., None] + y.abs()).reshape(shape)
        A["z1"] = A_z1
    if gout is None:
        return out, A
    g = _f(gout, dtype)[keep].reshape(n, C, -1)
    ds = (g * xs).sum(-1)
    f = s * (1 - s)
    dz2 = ds * f
    gW2 = dz2.T @ h
    dh = dz2 @ W2
    gate = (z1 > 0).to(dtype)
    dz1 = dh * gate
    gW1 = dz1.T @ p
    dp = dz1 @ W1
    gx = g * s[..., None] + dp[..., None] / HW
    p1 = torch.zeros_like(gW1) if prior_w1 is None else _f(prior_w1, dtype)
    p2 = torch.zeros_like(gW2) if prior_w2 is None else _f(prior_w2, dtype)
    out.update(gx=gx.reshape(shape), gW1=gW1 + p1, gW2=gW2 + p2)
    if bounds:
        A_ds = 2 * (g * xs).abs().sum(-1)
        A_f = A_s * (1 - s) + s * (A_s + (1 - s)) + f
        A_dz2 = A_ds * f + ds.abs() * A_f + dz2.abs()
        A["gW2"] = (A_dz2.T @ h.abs() + dz2.abs().T @ A_z1 + dz2.abs().T @ h.abs()) + p2.abs() + out["gW2"].abs()
        A_dz1 = ((A_dz2 + dz2.abs()) @ aW2) * gate
        A["gW1"] = (A_dz1.T @ p.abs() + dz1.abs().T @ A_p + dz1.abs().T @ p.abs()) + p1.abs() + out["gW1"].abs()
        A_dp = (A_dz1 + dz1.abs()) @ aW1
        A["gx"] = (g.abs() * A_s[..., None] + (g * s[..., None]).abs() + (A_dp + dp.abs())[..., None] / HW + gx.abs()).reshape(shape)
    return out, A


def push_off_se_kink(x, W1, valid=None, rounds=8):
    """W1 (float32) nudged until every hidden pre-activation z1 of the real frames has |z1| > KINK u A_z1 (a handful of
    values per frame: row k of W1 moves along the pooled vector of the offending frame).  Returns (W1, rounds used)."""
    W1 = W1.clone()
    W2 = torch.zeros(W1.shape[1], W1.shape[0])
    for it in range(rounds + 1):
        o, A = se_ref(x, W1, W2, valid)
        bad = o["z1"].abs() <= KINK * U * A["z1"]
        if not bool(bad.any()):
            return W1, it
        assert it < rounds, f"push_off_se_kink: {int(bad.sum())} hidden units still on the kink after {rounds} rounds"
        keep = torch.ones(x.shape[0], dtype=torch.bool) if valid is None else valid.bool().cpu()
        p = x[keep].double().flatten(2).mean(-1)
        W = W1.double()
        for f_, k in bad.nonzero().tolist():
            sgn = 1.0 if float(o["z1"][f_, k]) >= 0 else -1.0
            W[k] += sgn * 4 * KINK * U * float(A["z1"][f_, k]) * p[f_] / float(p[f_] @ p[f_])
        W1 = W.float()
    raise AssertionError("unreachable")


# ------------------------------------------------------------------------------------------------ temporal aggregation
def bilinear_matrix(n_in, n_out, align_corners=False, dtype=torch.float64):
    """[n_out, n_in] weights of torch's bilinear upsampling along one axis, written out from area_pixel_compute_source_index:
    src = max(0, (in / out) (dst + 0.5) - 0.5), taps floor(src) and min(floor(src) + 1, in - 1), weights 1 - frac and frac.
    align_corners=True (src = dst (in - 1) / (out - 1)) exists for the checker's own tests."""
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for dst in range(n_out):
        if n_in == n_out:
            M[dst, dst] = 1.0
            continue
        if align_corners:
            src = dst * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        else:
            src = max(0.0, (n_in / n_out) * (dst + 0.5) - 0.5)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        w1 = src - i0
        M[dst, i0] += 1.0 - w1
        M[dst, i1] += w1
    return M.to(dtype)


def agg_ref(x, attn, valid, gout=None, mode="att_group", prior_gx=None, prior_gattn=None, n_head=None, dtype=torch.float64,
            bounds=True, align_corners=False, cpg=None):
    """Temporal aggregation out[b, g cpg + c] = sum_t up(w[g,b,t]) keep[b,t] x[b,t, g cpg + c] and its backward at gout.

    x [B,T,C,H,W]; attn [n_head,B,T,h,w] (mode "mean": None, pass n_head); valid [B,T] bool or None.  w = attn
    ("att_group"), the head mean repeated for every group ("att_mean"), or keep / #valid frames of b as a 1x1 map ("mean").
    up = bilinear, align_corners=False, as the matrices of bilinear_matrix().  prior_gx / prior_gattn: gradients already on x
    / attn (the kernels add to them; on padded frames a prior on x stays as it is, without one gx is 0).
    align_corners / cpg (channels per group, default C / n_head): wrong settings for the checker's own tests.

    Returns out [B,C,H,W], gx [B,T,C,H,W] (every frame), gattn like attn (every frame; not for "mean").  Every step is
    linear in each operand: the bound is the same map on absolute values (as conv_ref.py), plus the rounding of results."""
    bounds = bounds and dtype == torch.float64
    x = _f(x, dtype)
    B, T, C, H, W = x.shape
    keep = torch.ones(B, T, dtype=torch.bool) if valid is None else valid.bool().cpu().view(B, T)
    kf = keep.to(dtype)
    x = torch.where(keep[:, :, None, None, None], x, torch.zeros((), dtype=dtype))       # padded frames are never read
    if mode == "mean":
        nh = n_head
        w = (kf / kf.sum(1, keepdim=True))[None].expand(nh, B, T)[..., None, None].contiguous()
        A_w = w.clone()                                           # the division
    else:
        attn = _f(attn, dtype)
        nh = attn.shape[0]
        if mode == "att_mean":
            w = attn.mean(0, keepdim=True).expand_as(attn)
            A_w = attn.abs().mean(0, keepdim=True).expand_as(attn) + w.abs()
        else:
            w, A_w = attn, torch.zeros_like(attn)
    zero = torch.zeros((), dtype=dtype)
    w = torch.where(keep[None, :, :, None, None], w, zero)          # padded frames of attn are never read either
    A_w = torch.where(keep[None, :, :, None, None], A_w, zero)
    h_, w_ = w.shape[-2:]
    Uy, Ux = bilinear_matrix(h_, H, align_corners, dtype), bilinear_matrix(w_, W, align_corners, dtype)
    up = lambda t: torch.einsum("Yi,gbtij,Xj->gbtYX", Uy, t, Ux)          # noqa: E731
    down = lambda t: torch.einsum("Yi,gbtYX,Xj->gbtij", Uy, t, Ux)        # noqa: E731
    a = up(w) * kf[None, :, :, None, None]
    cpg = C // nh if cpg is None else cpg
    ng = C // cpg
    gsel = torch.arange(ng) % nh                                  # head of channel group (identity unless cpg is wrong)
    x6 = x.view(B, T, ng, cpg, H, W)
    ag = a[gsel]
    outv = torch.einsum("gbtYX,btgcYX->bgcYX", ag, x6).reshape(B, C, H, W)
    out, A = {"out": outv}, {}
    if bounds:
        # the four taps: two products and two sums deep (4 |a|, on absolute values); out: the product and the sum over t
        A_a = up(A_w + 4 * w.abs()) * kf[None, :, :, None, None]
        A["out"] = torch.einsum("gbtYX,btgcYX->bgcYX", A_a[gsel] + 2 * ag.abs(), x6.abs()).reshape(B, C, H, W)
    if gout is None:
        return out, A
    go = _f(gout, dtype).view(B, ng, cpg, H, W)
    gx = torch.einsum("gbtYX,bgcYX->btgcYX", ag, go).reshape(B, T, C, H, W)
    pg = None if prior_gx is None else _f(prior_gx, dtype)
    if pg is not None:
        gx = torch.where(keep[:, :, None, None, None], gx + pg, pg)
    out["gx"] = gx
    gup = torch.einsum("btgcYX,bgcYX->gbtYX", x6, go)
    fold = lambda t: t if ng == nh else t.view(ng // nh, nh, *t.shape[1:]).sum(0)      # noqa: E731  (ng != nh: a planted fault)
    gup = fold(gup)
    gw = down(gup)
    if mode == "att_mean":
        gw = gw.mean(0, keepdim=True).expand_as(gw)
    pa = None if prior_gattn is None else _f(prior_gattn, dtype)
    if mode != "mean":
        out["gattn"] = gw if pa is None else gw + pa
    if bounds:
        A_gx = torch.einsum("gbtYX,bgcYX->btgcYX", (A_a + a.abs())[gsel], go.abs()).reshape(B, T, C, H, W)
        if pg is not None:
            A_gx = torch.where(keep[:, :, None, None, None], A_gx + pg.abs() + gx.abs(), torch.zeros((), dtype=dtype))
        A["gx"] = A_gx
        if mode != "mean":
            A_gup = fold(2 * torch.einsum("btgcYX,bgcYX->gbtYX", x6.abs(), go.abs()))
            A_gw = down(A_gup + 4 * gup.abs())
            if mode == "att_mean":
                A_gw = A_gw.mean(0, keepdim=True).expand_as(A_gw) + gw.abs()
            A["gattn"] = A_gw if pa is None else A_gw + pa.abs() + out["gattn"].abs()
    return out, A


# ------------------------------------------------------------------------------------------------ dropout + per-pixel GroupNorm
def pixel_gn_ref(x, keep_mask, p, gamma, beta, groups, gout=None, eps=1e-5, dtype=torch.float64, bounds=True):
    """The L-TAE MLP tail: xd = x keep / (1 - p) (keep [B*HW, C], pixel-major like the reference's [P,C] activations; None
    or p = 0: no dropout), then GroupNorm over the C / groups channels of each group of each pixel, and the backward at gout
    through both.  Returns y, gx [B,C,...], dgamma, dbeta [C].  The statistics formulas and bounds are those of
    _norm_core over the channel axis of a group; rsqrtf carries RSQRT_ULPS; the dropout scale carries 2 |xd| (the rounded
    1 / (1 - p) and the product)."""
    bounds = bounds and dtype == torch.float64
    xs = _f(x, dtype)
    shape = xs.shape
    B, C = shape[:2]
    xs = xs.reshape(B, C, -1)
    HW = xs.shape[-1]
    cpg = C // groups
    if keep_mask is not None and p > 0:
        sc = _f(keep_mask, dtype).view(B, HW, C).permute(0, 2, 1) / (1.0 - p)
    else:
        sc = torch.ones(B, C, HW, dtype=dtype)
    xd = xs * sc
    v4 = lambda t: t.reshape(B, groups, cpg, HW)      # noqa: E731
    g = None if gout is None else v4(_f(gout, dtype).reshape(B, C, HW))
    gam, bet = _f(gamma, dtype).view(1, groups, cpg, 1), _f(beta, dtype).view(1, groups, cpg, 1)
    A_in = 2 * v4(xd).abs() if bounds else None
    o, A = _norm_core(v4(xd), gam, bet, (2,), (0, 3), eps, False, None, g, None, "two_pass", RSQRT_ULPS, A_in, bounds)
    out = {"y": o["y"].reshape(shape)}
    Aout = {"y": A["y"].reshape(shape)} if bounds else {}
    if gout is not None:
        out.update(gx=(o["gx"].reshape(B, C, HW) * sc).reshape(shape), dgamma=o["dgamma"].reshape(C), dbeta=o["dbeta"].reshape(C))
        if bounds:
            Aout.update(gx=((A["gx"].reshape(B, C, HW) + 2 * o["gx"].reshape(B, C, HW).abs()) * sc).reshape(shape),
                        dgamma=A["dgamma"].reshape(C), dbeta=A["dbeta"].reshape(C))
    return out, Aout


# ================================================================================================ row tables and inputs
# One table per kernel file, shared by tests/test_norm_reference.py (fp32 evaluation of every row, kink builder) and
# tests/test_norm_reference_gpu.py (the kernels).  `cus` sizes the rows whose point is a grid that wraps.
SEG = 2048


def two_pass_branches(HW):
    """Branches of the two-pass kernels of csrc/norm.hip (and se.hip) that a plane of HW floats reaches, with the arithmetic
    of seg_len / n_segs: "full" (a 2048-float segment), "full_unaligned" (the same at a row base that is not 16-byte
    aligned), "float4_tail" (a shorter segment of a multiple of 4 floats), "scalar"."""
    L = min(HW, SEG)
    segs = (HW + L - 1) // L
    out = set()
    for s in range(segs):
        ln = min(HW - s * L, L)
        if ln == SEG:
            out.add("full" if HW % 4 == 0 else "full_unaligned")
        else:
            out.add("float4_tail" if ln % 4 == 0 else "scalar")
    return out


def onepass_instance(row, min_hw=256):
    """NK of the one-pass instance the row's shape takes (arithmetic of onepass_nk in csrc/norm.hip), or 0."""
    HW = row["H"] * row["W"]
    L = min(HW, SEG)
    if HW < min_hw or HW % L or L % 256 or L // 256 not in (1, 2, 4, 8):
        return 0
    batch = row["kind"] == "batch"
    if batch and (not row.get("training", True) or row.get("pad")):
        return 0
    wpg = (row["N"] if batch else row["C"] // row["groups"]) * (HW // L)
    if wpg > 512 or (wpg != 1 and wpg % 4):
        return 0
    return L // 256


def norm_rows(cus):
    q = math.ceil(2.5 * 8 * cus)                  # quads of the wrapping rows: 2.5 rounds of 8 workgroups per CU
    R = lambda name, kind, N, C, H, W, groups=4, **kw: dict(name=name, kind=kind, N=N, C=C, H=H, W=W, groups=groups, **kw)   # noqa: E731
    rows = [
        # ---- one-pass instances, GroupNorm
        R("g_nk1", "group", 3, 16, 16, 16, pad=[1]),
        R("g_nk1_res_one_wave", "group", 2, 8, 16, 16, groups=8, res=True),
        R("g_nk2_off30", "group", 3, 16, 16, 32, stats="off30"),
        R("g_nk2_res", "group", 3, 16, 16, 32, res=True, pad=[0], pad_value=-2.0),
        R("g_nk4_norelu", "group", 3, 16, 32, 32, relu=False, pad=[2]),
        R("g_nk4_res_noaffine", "group", 2, 16, 32, 32, res=True, affine=False),
        R("g_nk8_off1000", "group", 2, 8, 64, 64, groups=2, stats="off1000"),
        R("g_nk8_res_n1_gamma0", "group", 1, 16, 32, 64, res=True, gamma="zeros_neg"),
        R("g_limit_512_waves", "group", 1, 64, 256, 256),
        R("g_over_512_waves", "group", 1, 128, 256, 256),
        R("g_wpg3", "group", 2, 12, 32, 32),
        R("g_wrap_nk1_res", "group", math.ceil(4 * q / 64), 64, 16, 16, res=True, pad="every5"),
        R("g_frozen_producer_nk4", "group", 3, 16, 32, 32, frozen=True, pad=[1]),
        # ---- one-pass instances, BatchNorm
        R("b_nk1", "batch", 4, 8, 16, 16),
        R("b_nk1_res", "batch", 4, 8, 16, 16, res=True),
        R("b_nk2_off30", "batch", 4, 8, 16, 32, stats="off30"),
        R("b_nk2_res", "batch", 8, 4, 16, 32, res=True),
        R("b_nk4_one_wave", "batch", 1, 8, 32, 32),
        R("b_nk4_res_gamma0", "batch", 4, 8, 32, 32, res=True, gamma="zeros_neg"),
        R("b_nk8", "batch", 2, 4, 64, 64),
        R("b_nk8_res_norelu", "batch", 4, 4, 32, 64, res=True, relu=False),
        R("b_wrap_nk1", "batch", 4, q, 16, 16),
        R("b_wpg3", "batch", 3, 8, 32, 32),
        # ---- two-pass only
        R("b_flags", "batch", 5, 8, 32, 32, pad=[0, 3], res=True, pad_value=0.5),
        R("b_flags_3x3", "batch", 4, 8, 3, 3, pad=[1]),
        R("b_flags_47", "batch", 3, 4, 47, 47, pad=[1]),
        R("b_eval", "batch", 3, 8, 32, 32, training=False),
        R("b_eval_flags_res", "batch", 3, 8, 5, 5, training=False, pad=[2], res=True),
        R("b_cnt1", "batch", 1, 4, 1, 1),
        R("g_3x3", "group", 3, 8, 3, 3, pad=[2]),
        R("g_5x5_res", "group", 2, 8, 5, 5, res=True),
        R("g_6x6", "group", 2, 8, 6, 6),
        R("g_48_ragged", "group", 2, 8, 48, 48, pad=[0]),
        R("g_80_off30", "group", 1, 8, 80, 80, stats="off30"),
        R("g_96_res", "group", 2, 8, 96, 96, res=True, pad=[1]),
        R("g_47_unaligned_res", "group", 3, 8, 47, 47, res=True, pad=[0], pad_value=1.5),
        R("g_47_off1000_norelu", "group", 1, 4, 47, 47, groups=2, stats="off1000", relu=False),
        R("g_cnt1", "group", 2, 4, 1, 1),
        R("g_const_plane", "group", 2, 8, 8, 8, stats="const"),
        R("g_frozen_producer_5x5", "group", 2, 8, 5, 5, frozen=True),
        R("g_noaffine_3x3", "group", 2, 8, 3, 3, affine=False, pad=[0]),
    ]
    return rows


def _pad_list(row):
    pad = row.get("pad")
    if pad == "every5":
        return list(range(0, row["N"], 5))
    return list(pad or [])


def norm_offset(row):
    """|mean| / sigma of the row's input."""
    return {"off30": 30.0, "off1000": 1000.0}.get(row.get("stats", "plain"), 0.25)


def norm_inputs(row, seed=7):
    """CPU float32 inputs of a normalisation row; padded frames of x, res and gout hold NaN.  x is kink-free (push_off_kink;
    "kink_rounds" tells how many rounds that took)."""
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = row["N"], row["C"], row["H"], row["W"]
    stats = row.get("stats", "plain")
    x = torch.randn(N, C, H, W, generator=g)
    x = x + 30.0 if stats == "off30" else x + 1000.0 if stats == "off1000" else x * 2 + 0.5
    valid = torch.ones(N, dtype=torch.bool)
    valid[_pad_list(row)] = False
    if stats == "const":                 # a whole normalisation group constant: variance 0, rstd = 1 / sqrt(eps)
        if row["kind"] == "group":
            x[int(valid.nonzero()[0]), : C // row["groups"]] = 1.25
        else:
            x[:, 0] = 1.25
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    sgn = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    beta = sgn * (0.05 + 0.2 * torch.randn(C, generator=g).abs())
    if row.get("gamma") == "zeros_neg":
        gamma[0] = 0.0
        gamma[1::3] = -gamma[1::3].abs() - 0.25
        gamma[C - 1] = 0.0
    if not row.get("affine", True):
        gamma = beta = None
    res = torch.randn(N, C, H, W, generator=g) if row.get("res") else None
    gout = torch.randn(N, C, H, W, generator=g)
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if stats in ("off30", "off1000"):
        rm = rm + norm_offset(row)
    nan = float("nan")
    for t in (x, res, gout):
        if t is not None:
            t[~valid] = nan
    rounds = 0
    if row.get("relu", True):
        x, rounds = push_off_kink(x, gamma, beta, row["kind"], row["groups"], row.get("training", True), (rm, rv), valid)
    return dict(x=x, gamma=gamma, beta=beta, res=res, gout=gout, valid=valid, rm=rm, rv=rv, kink_rounds=rounds)


def norm_row_ref(row, t, dtype=torch.float64, **kw):
    return norm_ref(t["x"], t["gamma"], t["beta"], row["kind"], row["groups"], row.get("training", True), (t["rm"], t["rv"]),
                    t["res"], row.get("relu", True), t["valid"], t["gout"], dtype=dtype, **kw)


def norm_frob(row, name):
    """Frobenius bar of an output: those of tests/test_ops_gpu.py, unchanged, with one derived floor.  Any fp32 evaluation
    holds the group mean m only to u |m|, so every xhat of the group carries a common shift of up to u |m| / sigma, and with it
    y and dgamma = sum g' xhat (gx, dbeta, dbias and the statistics themselves do not: their relative error does not grow
    with the offset).  At |m| / sigma = 1000 that shift alone is 6e-5, above the bars, so there -- and only there -- y and
    dgamma get FROB + C_BOUND u |m| / sigma (1.2e-4 + the bar); at |m| / sigma = 30 the shift is 1.8e-6 and the bars stay
    as they are.  tests/test_norm_reference.py holds the fp32 evaluation of the formulas to exactly these bars.  No
    Frobenius bar (the bound alone) where the reference is identically zero and only rounding noise is left: dbias when a channel is a whole normalisation group or
    part of none that crosses channels (sum of gx over a group = 0: batch statistics, GroupNorm with one channel per
    group), and gx / dgamma / dbias of a group of one element (xhat = 0, gx = 0)."""
    batch = row["kind"] == "batch"
    own_group = (batch and row.get("training", True)) or (not batch and row["C"] == row["groups"])
    cnt = row["H"] * row["W"] * (row["N"] - len(_pad_list(row)) if batch else row["C"] // row["groups"])
    if (name == "dbias" and own_group) or (name in ("gx", "dgamma", "dbias") and cnt == 1 and not (batch and not row.get("training", True))):
        return float("inf")
    if name in ("y", "dgamma") and row.get("stats") == "off1000":
        return FROB[name] + C_BOUND * U * norm_offset(row)
    return FROB[name]


def se_rows():
    R = lambda name, N, C, H, W, **kw: dict(name=name, N=N, C=C, H=H, W=W, **kw)      # noqa: E731
    return [R("se_c16_3x3_scalar", 3, 16, 3, 3, pad=[1]),
            R("se_48_ragged_prior", 2, 32, 48, 48, prior=True),
            R("se_47_unaligned_padvalue", 3, 16, 47, 47, pad=[0], pad_value=-1.5),
            R("se_c1024_prior", 3, 1024, 4, 4, prior=True, pad=[2]),
            R("se_c64_32", 4, 64, 32, 32, pad=[1], pad_value=0.75),
            R("se_96_n1", 1, 16, 96, 96),
            R("se_c256_6x10", 2, 256, 6, 10, prior=True)]


def se_inputs(row, seed=17):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = row["N"], row["C"], row["H"], row["W"]
    x = torch.randn(N, C, H, W, generator=g) + (0.5 + torch.randn(N, C, 1, 1, generator=g))   # pooled values of order 1
    W1 = torch.randn(C // 16, C, generator=g) * 0.3
    W2 = torch.randn(C, C // 16, generator=g) * 0.5
    gout = torch.randn(N, C, H, W, generator=g)
    valid = torch.ones(N, dtype=torch.bool)
    valid[list(row.get("pad") or [])] = False
    x[~valid] = float("nan")
    gout[~valid] = float("nan")
    p1 = torch.randn(W1.shape, generator=g) if row.get("prior") else None
    p2 = torch.randn(W2.shape, generator=g) if row.get("prior") else None
    z1 = x[valid].double().flatten(2).mean(-1) @ W1.double().T
    dead = (z1 <= 0).all(0)                      # a hidden unit that no real frame switches on tests nothing behind it
    W1[dead] = -W1[dead]
    W1, rounds = push_off_se_kink(x, W1, valid)
    return dict(x=x, W1=W1, W2=W2, gout=gout, valid=valid, prior_w1=p1, prior_w2=p2, kink_rounds=rounds)


def se_row_ref(row, t, dtype=torch.float64):
    return se_ref(t["x"], t["W1"], t["W2"], t["valid"], t["gout"], t["prior_w1"], t["prior_w2"], dtype=dtype)


def agg_rows():
    R = lambda name, B, T, C, nh, H, W, h, w, **kw: dict(name=name, B=B, T=T, C=C, nh=nh, H=H, W=W, h=h, w=w, **kw)   # noqa: E731
    return [R("cpg1_ratio2", 2, 3, 16, 16, 16, 16, 8, 8, pad=[(0, 2)]),
            R("cpg2_ratio4_nonsquare", 2, 3, 32, 16, 16, 32, 4, 8, pad=[(1, 0)], prior_gattn=True),
            R("cpg4_ratio2x8", 1, 4, 64, 16, 16, 32, 8, 4, pad=[(0, 1)], prior_gx=True),
            R("cpg8_ratio1", 2, 3, 128, 16, 8, 8, 8, 8, pad=[(0, 0)]),
            R("cpg16_ratio8", 2, 2, 64, 4, 16, 16, 2, 2, prior_gx=True, prior_gattn=True, pad=[(1, 1)]),
            R("w256_adjoint", 1, 2, 16, 16, 8, 256, 4, 64),
            R("w128_adjoint", 1, 3, 16, 16, 8, 128, 2, 32, pad=[(0, 1)]),
            R("one_real_frame", 2, 4, 32, 16, 8, 8, 4, 4, pad=[(0, 0), (0, 1), (0, 3)]),
            R("no_gx", 2, 3, 32, 16, 8, 16, 4, 4, pad=[(1, 2)], need_x=False),
            R("no_gx_cpg1", 1, 3, 16, 16, 8, 8, 2, 2, need_x=False, prior_gattn=True),
            R("no_gattn", 2, 3, 64, 16, 8, 8, 4, 4, pad=[(0, 2)], need_a=False),
            R("mean", 2, 4, 32, 16, 8, 8, 1, 1, mode="mean", pad=[(0, 0), (0, 1), (0, 3)]),
            R("mean_gx_prior", 1, 3, 16, 16, 4, 8, 1, 1, mode="mean", prior_gx=True, pad=[(0, 1)]),
            R("att_mean", 2, 3, 32, 16, 16, 16, 4, 4, mode="att_mean", pad=[(1, 0)]),
            R("att_mean_accumulate", 2, 3, 64, 16, 8, 16, 4, 8, mode="att_mean", prior_gattn=True, prior_gx=True, pad=[(0, 2)])]


def agg_inputs(row, seed=23):
    g = torch.Generator().manual_seed(seed)
    B, T, C, nh, H, W, h, w = (row[k] for k in ("B", "T", "C", "nh", "H", "W", "h", "w"))
    x = torch.randn(B, T, C, H, W, generator=g)
    attn = torch.softmax(torch.randn(nh, B, T, h, w, generator=g), dim=2)
    gout = torch.randn(B, C, H, W, generator=g)
    valid = torch.ones(B, T, dtype=torch.bool)
    for b, t_ in row.get("pad") or []:
        valid[b, t_] = False
    x[~valid] = float("nan")
    if row.get("mode", "att_group") != "mean":
        attn[:, ~valid] = float("nan")
    pgx = torch.randn(B, T, C, H, W, generator=g) if row.get("prior_gx") else None
    pga = torch.randn(nh, B, T, h, w, generator=g) if row.get("prior_gattn") else None
    return dict(x=x, attn=attn, gout=gout, valid=valid, prior_gx=pgx, prior_gattn=pga)


def agg_row_ref(row, t, dtype=torch.float64, **kw):
    mode = row.get("mode", "att_group")
    return agg_ref(t["x"], None if mode == "mean" else t["attn"], t["valid"], t["gout"], mode, t["prior_gx"],
                   t["prior_gattn"], row["nh"], dtype=dtype, **kw)


def pixel_gn_rows():
    return [dict(name="c128_8x8", B=2, C=128, H=8, W=8, groups=16, p=0.2),
            dict(name="c64_5x7_hw_not_64", B=1, C=64, H=5, W=7, groups=16, p=0.5),
            dict(name="c256_cpg16", B=2, C=256, H=4, W=4, groups=16, p=0.1),
            dict(name="c64_hw200_chunks", B=2, C=64, H=10, W=20, groups=16, p=0.3),
            dict(name="c32_no_dropout", B=1, C=32, H=3, W=3, groups=16, p=0.0)]


def pixel_gn_inputs(row, seed=19):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = row["B"], row["C"], row["H"], row["W"]
    x = torch.randn(B, C, H, W, generator=g)
    gamma = 1 + 0.3 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    keep = (torch.rand(B * H * W, C, generator=g) >= row["p"]).float()
    gout = torch.randn(B, C, H, W, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, keep=keep, gout=gout)


def pixel_gn_row_ref(row, t, dtype=torch.float64):
    return pixel_gn_ref(t["x"], t["keep"], row["p"], t["gamma"], t["beta"], row["groups"], t["gout"], dtype=dtype)
