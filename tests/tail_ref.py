"""Independent float64 references of the training tail, each with a per-element error bound (CPU only): cross entropy
focal CE and smooth CE of csrc/loss.hip, flat Adam of csrc/misc.hip, the metrics pass, confusion_add, boundary_target and
region_relabel of csrc/metrics.hip.

Every floating-point reference is written out as explicit formulas (forward and backward, no autograd, no
F.cross_entropy; tests/test_tail_reference.py ties them to those), each line next to its bound.  A reference returns
({name: value}, {name: A}) like norm_ref.norm_ref, and a kernel result must satisfy

    |got - ref64| <= C_BOUND * u * A + 1e-30,     u = 2^-24,     C_BOUND = 2 for every output,

element by element (conv_ref.assert_within).  A is first-order propagation of per-operation rounding; C_BOUND = 2 is that
plus a margin for second-order terms and is NOT fitted to the kernels: the same formulas evaluated with
dtype=torch.float32 must stay <= 1 on every row of the GPU tables (test_tail_reference.py::test_fp32_evaluation_*).  A kernel
that legitimately needs more gets a named term in A, never a larger constant.  The named terms, in ulp of the result
(1 ulp = 2 u), all at the project's starting value for un-measured intrinsics:

    EXP_ULPS = 2    exp of the max-subtracted logits and of log pt
    LOG_ULPS = 2    log of the softmax denominator
    POW_ULPS = 2    (1 - pt)^gamma of the focal loss, beta^step of Adam

The cross-entropy kernels use the fast __expf / __logf, the focal and smooth kernels expf / logf.  The intrinsics were kept
and run under the SAME terms: on an MI355X the cross-entropy rows stayed below ratio 1 with EXP_ULPS = LOG_ULPS = 2 (table in
tests/test_tail_reference_gpu.py), so neither a separate term nor a change of the kernels was needed.

Softmax pieces (z the logits of a pixel, linear steps carry the same map on absolute values as in conv_ref.py):

    d = z - max z;  e = exp(d)          A_e   = (2 EXP_ULPS + |d|) e          (|d|: rounding of the argument, as in ltae_ref)
    s = sum_k e                         A_s   = sum A_e + s                    (the K-term sum: sum |terms|)
    L = log s                           A_L   = A_s / s + 2 LOG_ULPS |L|
    p = e / s                           A_p   = A_e / s + e A_s / s^2 + 2 p    (1 / s, then the product)
    lse = max z + L                     A_lse = A_L + |lse|

Block partials are float and the finalise step is double: a total of pixel terms carries sum A_term + 2 sum |term|.

Focal CE, gamma < 1: d/d(om) of om^gamma is unbounded at om = 1 - pt -> 0, so the bound of the pow terms is the interval form
max |f(om +- u A_om) - f(om)| / u with the interval clamped at 0, not the derivative.  For om^(gamma - 1) the clamp is at u, the
smallest positive 1 - pt that exists in float32, and om = 0 itself takes the finite limit of the whole first term of the
derivative, gamma om^(gamma-1) pt log pt -> 0 (log pt ~ -om), as focal_bwd_kernel does (the plain expression is inf * 0 =
NaN there for every gamma < 1).  No element is left out.

Adam: the hyper-parameters are taken as their float32 values widened to float64 (the kernel receives floats).  The bias
corrections 1 - b^step carry their cancellation, A_bc = 2 POW_ULPS b^step + bc.  The update p_new - p_old is an output of its
own: the step is 1e-3 of p, so on p a mis-scaled step hides under u |p|; the rows keep |p| small enough for the update
to be resolved.

The integer kernels are restated in numpy and compared bit for bit.

Nothing here imports crop2seg_amd or oracle.
"""
import numpy as np
import torch

from conv_ref import U, assert_within, bound_ratio  # noqa: F401  (re-exported: the tests take them from here)

C_BOUND = 2.0
EXP_ULPS = 2.0
LOG_ULPS = 2.0
POW_ULPS = 2.0
# the bars of tests/test_ops_gpu.py and tests/test_tail_gpu.py (never looser than those)
SCALAR_REL = 4e-6            # |loss - ref| <= SCALAR_REL * |ref|
GRAD_MAX_REL = 4e-6          # max |g - ref| <= GRAD_MAX_REL * max |ref|
ADAM_FROB = 1e-6             # Frobenius of p, m, v after a step


def _f(t, dtype):
    return None if t is None else torch.as_tensor(t).detach().to(dtype).cpu()


def _rows(logits, dtype):
    """[B,K,H,W] -> [B*H*W, K] in the kernels' pixel order e = b * HW + pix."""
    B, K = logits.shape[:2]
    return _f(logits, dtype).reshape(B, K, -1).permute(0, 2, 1).reshape(-1, K)


def _nchw(g, shape):
    B, K = shape[:2]
    return g.reshape(B, -1, K).permute(0, 2, 1).reshape(shape)


def _softmax(z, bounds):
    mx = z.max(1, keepdim=True).values
    d = z - mx
    e = torch.exp(d)
    s = e.sum(1, keepdim=True)
    L = torch.log(s)
    p = e / s
    o = {"mx": mx, "d": d, "e": e, "s": s, "L": L, "p": p, "lse": mx + L}
    A = {}
    if bounds:
        A["e"] = (2 * EXP_ULPS + d.abs()) * e
        A["s"] = A["e"].sum(1, keepdim=True) + s
        A["L"] = A["s"] / s + 2 * LOG_ULPS * L.abs()
        A["p"] = A["e"] / s + e * A["s"] / s ** 2 + 2 * p
        A["lse"] = A["L"] + o["lse"].abs()
    return o, A


def _total(terms, A_terms):
    """Sum of per-pixel terms (float block partials, double finalise) and its bound."""
    return terms.sum(), (None if A_terms is None else A_terms.sum() + 2 * terms.abs().sum())


# ------------------------------------------------------------------------------------------------ cross entropy
def ce_ref(logits, target, class_w=None, label_smoothing=0.0, ignore_index=-100, dtype=torch.float64, bounds=True,
           fault=None):
    """nn.CrossEntropyLoss(weight, label_smoothing, ignore_index), reduction mean, and d loss / d logits.  Targets outside
    [0, K) other than ignore_index are skipped and counted.  Returns loss [1], glogits [B,K,H,W], bad [1], tot [2] (the sum of
    the pixel terms and the sum of the target weights: the workspace tail).

        nll_k = lse - z_k                               A_nll = A_lse + |nll_k|
        l = w_y nll_y                                   A_l   = w_y A_nll_y + |l|
        sm = sum_k w_k nll_k                            A_sm  = sum w_k A_nll_k + 2 sum |w_k nll_k|
        li = (1-eps) l + (eps/K) sm                     A_li  = (1-eps) (A_l + 2 |l|) + (eps/K) (A_sm + 3 |sm|) + |li|
        num = sum li;  den = sum w_y                    _total();  A_den = 2 den
        loss = num / den                                A     = A_num / den + |num| A_den / den^2 + |loss|
        rd = 1 / den                                    A_rd  = (A_den + 2 den) / den^2       (den to float, then 1 / den)
        w' = w_y rd                                     A_w'  = w_y A_rd + w'
        eps = 0:  g_k = w' (p_k - [k=y])                A_g   = A_w' |p - 1| + w' (A_p + |p - 1|) + |g|
        eps > 0:  a = (1-eps) w';  c = (eps/K) rd;  W = sum_k w_k
                  g_k = a (p_k - [k=y]) + c (W p_k - w_k)     each product and sum as above

    fault (for the checker's own tests): "last_class" p of class K-1 taken from class K-2; "smooth_k" eps / (K-1); "partial"
    the 256 pixels from 131072 on missing from the totals."""
    bounds = bounds and dtype == torch.float64
    shape = tuple(logits.shape)
    K = shape[1]
    z = _rows(logits, dtype)
    t = torch.as_tensor(target).reshape(-1).long().cpu()
    cw = torch.ones(K, dtype=dtype) if class_w is None else _f(class_w, dtype)
    eps = float(np.float32(label_smoothing))
    skip = (t == ignore_index) | (t < 0) | (t >= K)
    bad = ((t != ignore_index) & ((t < 0) | (t >= K))).sum()
    keep = ~skip
    y = t.clamp(0, K - 1)
    o, A = _softmax(z, bounds)
    onehot = torch.zeros_like(z).scatter_(1, y[:, None], 1.0)
    nll = o["lse"] - z
    wy = cw[y]
    l0 = wy * nll.gather(1, y[:, None])[:, 0]
    ek = eps / (K - 1 if fault == "smooth_k" and K > 1 else K)
    sm = (cw * nll).sum(1)
    li = (1 - eps) * l0 + ek * sm if eps > 0 else l0
    li = torch.where(keep, li, torch.zeros_like(li))
    wk = torch.where(keep, wy, torch.zeros_like(wy))
    inc = torch.ones_like(li)
    if fault == "partial":
        inc[131072:131072 + 256] = 0
    num, den = (li * inc).sum(), (wk * inc).sum()
    loss = num / den
    p = o["p"]
    if fault == "last_class" and K > 1:
        p = p.clone()
        p[:, K - 1] = p[:, K - 2]
    rd = 1.0 / den
    w1 = wy * rd
    W = cw.sum()
    if eps > 0:
        a, c = (1 - eps) * w1, ek * rd
        t1, inner = a[:, None] * (p - onehot), W * p - cw
        g = t1 + c * inner
    else:
        g = w1[:, None] * (p - onehot)
    g = torch.where(keep[:, None], g, torch.zeros_like(g))
    out = {"loss": loss.reshape(1), "glogits": _nchw(g, shape), "bad": bad.to(dtype).reshape(1),
           "tot": torch.stack([num, den])}
    if not bounds:
        return out, {}
    A_nll = A["lse"] + nll.abs()
    A_l0 = wy * A_nll.gather(1, y[:, None])[:, 0] + l0.abs()
    if eps > 0:
        A_sm = (cw * A_nll).sum(1) + 2 * (cw * nll).abs().sum(1)
        A_li = (1 - eps) * (A_l0 + 2 * l0.abs()) + ek * (A_sm + 3 * sm.abs()) + li.abs()
    else:
        A_li = A_l0
    A_li = torch.where(keep, A_li, torch.zeros_like(A_li))
    _, A_num = _total(li, A_li)
    A_den = 2 * den
    A_loss = A_num / den + num.abs() * A_den / den ** 2 + loss.abs()
    A_rd = (A_den + 2 * den) / den ** 2
    A_w1 = wy * A_rd + w1
    pm = (p - onehot).abs()
    if eps > 0:
        A_a = (1 - eps) * (A_w1 + 2 * w1)
        A_c = ek * (A_rd + 3 * rd)
        A_W = 2 * cw.abs().sum()
        A_t1 = A_a[:, None] * pm + a[:, None] * (A["p"] + pm) + t1.abs()
        A_in = A_W * p + W * A["p"] + (W * p).abs() + inner.abs()
        A_g = A_t1 + A_c * inner.abs() + c * A_in + (c * inner).abs() + g.abs()
    else:
        A_g = A_w1[:, None] * pm + w1[:, None] * (A["p"] + pm) + g.abs()
    A_g = torch.where(keep[:, None], A_g, torch.zeros_like(A_g))
    zero = torch.zeros(1, dtype=dtype)
    return out, {"loss": A_loss.reshape(1), "glogits": _nchw(A_g, shape), "bad": zero,
                 "tot": torch.stack([A_num + num.abs(), A_den + den])}


# ------------------------------------------------------------------------------------------------ focal CE
def _pow_interval(om, A_om, expo, floor):
    """Interval bound of om^expo in units of u: max |f(om +- u A_om) - f(om)| / u, the interval clamped at `floor`."""
    f = lambda x: torch.pow(x, expo)      # noqa: E731
    lo, hi = (om - U * A_om).clamp_min(floor), (om + U * A_om).clamp_min(floor)
    f0 = f(om.clamp_min(floor))
    return torch.maximum((f(lo) - f0).abs(), (f(hi) - f0).abs()) / U + 2 * POW_ULPS * f0.abs()


def focal_ref(logits, target, gamma=1.0, ignore_index=-100, class_w=None, size_average=True, prior=None,
              dtype=torch.float64, bounds=True, fault=None):
    """FocalCELoss(gamma, size_average, ignore_index, weight) as csrc/loss.hip states it: unweighted the mean / sum over the
    kept pixels of f = -(1 - pt)^gamma log pt, weighted the product of the mean / sum of w[target] and the mean / sum of f;
    `prior`: the loss the value is added to.  Returns loss [1], glogits, tot [3] = (sum f, #kept, d loss / d sum f).

        lpt = (z_t - max z) - L                         A_lpt = |d_t| + A_L + |lpt|
        pt = exp(lpt);  om = 1 - pt                     A_pt  = (2 EXP_ULPS + A_lpt) pt;  A_om = A_pt + om
        pw = om^gamma                                   A_pw  = interval form (module docstring)
        f = -pw lpt                                     A_f   = A_pw |lpt| + pw A_lpt + |f|
        num = sum f;  cnt;  ws = sum w_t                _total();  A_ws = 2 ws
        scale = 1 | 1/cnt | ws | ws/cnt^2               A_sc  = scale A_ws / ws   (double; + scale once it is a float)
        loss = num scale (+ prior)                      A     = A_num scale + |num| A_sc + |loss| (+ |prior| + |sum|)
        q = om^(gamma-1);  t1 = gamma q pt lpt          A_t1  = gamma (A_q pt |lpt| + q A_pt |lpt| + q pt A_lpt) + 3 |t1|
                                                        (om = 0 or gamma = 0: t1 = 0, the limit; an interval that reaches 0
                                                        also admits that value: A_t1 >= |t1| / u)
        coef = (t1 - pw) scale                          A_cf  = (A_t1 + A_pw + |t1 - pw|) scale + |t1 - pw| (A_sc + scale) + |coef|
        g_k = coef ([k=t] - p_k)                        A_g   = A_cf |[k=t] - p| + |coef| (A_p + |[k=t] - p|) + |g|

    fault: "no_t1" coef without the gamma pt log pt term."""
    bounds = bounds and dtype == torch.float64
    shape = tuple(logits.shape)
    K = shape[1]
    z = _rows(logits, dtype)
    t = torch.as_tensor(target).reshape(-1).long().cpu()
    gamma = float(np.float32(gamma))
    keep = ~((t == ignore_index) | (t < 0) | (t >= K))
    y = t.clamp(0, K - 1)
    o, A = _softmax(z, bounds)
    onehot = torch.zeros_like(z).scatter_(1, y[:, None], 1.0)
    dt = o["d"].gather(1, y[:, None])[:, 0]
    lpt = dt - o["L"][:, 0]
    pt = torch.exp(lpt)
    om = (1 - pt).clamp_min(0)
    pw = torch.pow(om, gamma)
    f = torch.where(keep, -pw * lpt, torch.zeros_like(pw))
    kf = keep.to(dtype)
    num, cnt = f.sum(), kf.sum()
    weighted = class_w is not None
    cw = _f(class_w, dtype) if weighted else torch.ones(K, dtype=dtype)
    ws = (cw[y] * kf).sum()
    if weighted:
        scale = ws / (cnt * cnt) if size_average else ws
    else:
        scale = 1.0 / cnt if size_average else torch.ones((), dtype=dtype)
    l = num * scale
    loss = l if prior is None else _f(prior, dtype).reshape(()) + l
    live = (om > 0) & (gamma > 0)
    q = torch.pow(torch.where(live, om, torch.ones_like(om)), gamma - 1)
    t1 = torch.where(live, gamma * q * pt * lpt, torch.zeros_like(q))
    if fault == "no_t1":
        t1 = torch.zeros_like(t1)
    raw = t1 - pw
    coef = raw * scale
    dk = onehot - o["p"]
    g = torch.where(keep[:, None], coef[:, None] * dk, torch.zeros_like(dk))
    out = {"loss": loss.reshape(1), "glogits": _nchw(g, shape), "tot": torch.stack([num, cnt, scale])}
    if not bounds:
        return out, {}
    A_lpt = dt.abs() + A["L"][:, 0] + lpt.abs()
    A_pt = (2 * EXP_ULPS + A_lpt) * pt
    A_om = A_pt + om
    A_pw = _pow_interval(om, A_om, gamma, 0.0) if gamma > 0 else torch.zeros_like(om)
    A_f = torch.where(keep, A_pw * lpt.abs() + pw * A_lpt + f.abs(), torch.zeros_like(f))
    _, A_num = _total(f, A_f)
    A_sc = scale * 2 if weighted else torch.zeros((), dtype=dtype)
    A_l = A_num * scale + num.abs() * A_sc + l.abs()
    A_loss = A_l if prior is None else A_l + _f(prior, dtype).abs().reshape(()) + loss.abs()
    if gamma > 0:
        A_q = _pow_interval(om, A_om, gamma - 1, U if gamma < 1 else 0.0)
        qq = torch.pow(om.clamp_min(U if gamma < 1 else 0.0), gamma - 1)
        A_t1 = gamma * (A_q * pt * lpt.abs() + qq * A_pt * lpt.abs() + qq * pt * A_lpt) + 3 * t1.abs()
        if gamma < 1:
            A_t1 = torch.where(om - U * A_om <= 0, torch.maximum(A_t1, t1.abs() / U), A_t1)
    else:
        A_t1 = torch.zeros_like(om)
    A_cf = (A_t1 + A_pw + raw.abs()) * scale + raw.abs() * (A_sc + scale) + coef.abs()
    A_g = A_cf[:, None] * dk.abs() + coef.abs()[:, None] * (A["p"] + dk.abs()) + g.abs()
    A_g = torch.where(keep[:, None], A_g, torch.zeros_like(A_g))
    return out, {"loss": A_loss.reshape(1), "glogits": _nchw(A_g, shape),
                 "tot": torch.stack([A_num + num.abs(), torch.zeros((), dtype=dtype), A_sc + scale])}


# ------------------------------------------------------------------------------------------------ smooth CE 2D
def class_masks(target, K, fault=None):
    """[B,H,W] labels -> bool [B,H,W,K]: the classes at a pixel or its four neighbours (zero padding: pixels outside the
    image and labels outside [0, K) contribute nothing).  fault: "batch" the upper / lower neighbours are also taken from the
    flattened label array, across batch entries; "bit31" class 31 never enters the set."""
    t = torch.as_tensor(target).long().cpu()
    B, H, W = t.shape
    ok = (t >= 0) & (t < K)
    oh = torch.zeros(B, H, W, K + 1, dtype=torch.bool).scatter_(3, torch.where(ok, t, torch.full_like(t, K))[..., None], True)
    oh = oh[..., :K]
    m = oh.clone()
    m[:, 1:] |= oh[:, :-1]
    m[:, :-1] |= oh[:, 1:]
    if fault == "batch":
        flat, mf = oh.reshape(-1, K), m.reshape(-1, K)
        mf[W:] |= flat[:-W]
        mf[:-W] |= flat[W:]
        m = mf.reshape(B, H, W, K)
    m[:, :, 1:] |= oh[:, :, :-1]
    m[:, :, :-1] |= oh[:, :, 1:]
    if fault == "bit31" and K == 32:
        m[..., 31] = False
    return m, ok


def smooth_ref(logits, target, label_smoothing=0.1, class_w=None, bg=None, bg_index=0, reduction="mean",
               dtype=torch.float64, bounds=True, fault=None):
    """SmoothCrossEntropy2D: soft targets from the class set of class_masks, the fixed distribution `bg` at pixels labelled
    bg_index, CE with probability targets and class weights; mean over ALL B*H*W pixels / sum / none.  A label outside [0, K)
    is counted, its pixel contributes nothing.  Returns pixel_loss [B,H,W], loss [1] (mean, or the sum for sum / none),
    glogits (of that value), tot [2] = (sum of the pixel terms, bad labels).

        eps = ls / K                                    A_eps = eps
        es = eps (K - n);  el = (1 - es) / n            A_es  = (K - n) A_eps + es;  A_el = (A_es + |1 - es|) / n + el
        tk = el | eps | bg_k;  wt = w_k tk              A_wt  = w_k A_tk + wt
        lp_k = z_k - lse                                A_lp  = A_lse + |lp_k|
        pl = -sum_k wt lp_k                             A_pl  = sum (A_wt |lp| + wt A_lp) + 2 sum |wt lp|
        S = sum_k wt                                    A_S   = sum A_wt + S
        g_k = (p_k S - wt_k) / n_pix                    A_g   = (A_p S + p A_S + |p S| + A_wt + |p S - wt|) / n_pix + 2 |g|"""
    bounds = bounds and dtype == torch.float64
    shape = tuple(logits.shape)
    B, K, H, W = shape
    z = _rows(logits, dtype)
    t = torch.as_tensor(target).long().cpu()
    mask, ok = class_masks(t, K, fault)
    mask, ok, tf = mask.reshape(-1, K), ok.reshape(-1), t.reshape(-1)
    ls = float(np.float32(label_smoothing))
    eps = torch.tensor(ls, dtype=dtype) / K
    n = mask.sum(1).clamp_min(1).to(dtype)[:, None]
    es = eps * (K - n)
    el = (1 - es) / n
    tk = torch.where(mask, el, eps.expand_as(el))
    is_bg = torch.zeros_like(ok)
    if bg is not None:
        is_bg = ok & (tf == bg_index)
        tk = torch.where(is_bg[:, None], _f(bg, dtype)[None, :].expand_as(tk), tk)
    cw = torch.ones(K, dtype=dtype) if class_w is None else _f(class_w, dtype)
    wt = cw * tk
    o, A = _softmax(z, bounds)
    lp = z - o["lse"]
    pl = torch.where(ok, -(wt * lp).sum(1), torch.zeros_like(ok, dtype=dtype))
    S = wt.sum(1, keepdim=True)
    npix = float(B * H * W) if reduction == "mean" else 1.0
    inner = o["p"] * S - wt
    g = torch.where(ok[:, None], inner / npix, torch.zeros_like(inner))
    num = pl.sum()
    out = {"pixel_loss": pl.reshape(B, H, W), "loss": (num / npix).reshape(1), "glogits": _nchw(g, shape),
           "tot": torch.stack([num, (~ok).sum().to(dtype)])}
    if not bounds:
        return out, {}
    A_es = (K - n) * eps + es
    A_el = (A_es + (1 - es).abs()) / n + el
    A_tk = torch.where(mask, A_el, eps.expand_as(el))
    if bg is not None:
        A_tk = torch.where(is_bg[:, None], torch.zeros_like(A_tk), A_tk)
    A_wt = cw * A_tk + wt
    A_lp = A["lse"] + lp.abs()
    A_pl = torch.where(ok, (A_wt * lp.abs() + wt * A_lp).sum(1) + 2 * (wt * lp).abs().sum(1), torch.zeros_like(pl))
    A_S = A_wt.sum(1, keepdim=True) + S
    A_g = (A["p"] * S + o["p"] * A_S + (o["p"] * S).abs() + A_wt + inner.abs()) / npix + 2 * g.abs()
    A_g = torch.where(ok[:, None], A_g, torch.zeros_like(A_g))
    _, A_num = _total(pl, A_pl)
    return out, {"pixel_loss": A_pl.reshape(B, H, W), "loss": (A_num / npix + (num / npix).abs()).reshape(1),
                 "glogits": _nchw(A_g, shape), "tot": torch.stack([A_num + num.abs(), torch.zeros((), dtype=dtype)])}


# ------------------------------------------------------------------------------------------------ Adam
def adam_ref(p, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0, dtype=torch.float64, bounds=True,
             fault=None):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on flat tensors, the gradient scaled by grad_scale first.
    Returns m, v, p (the new values) and upd = p_new - p_old.

        gg = g gs                                       A_gg  = |gg|
        c1 = 1 - b1;  mm = b1 m + c1 gg                 A_mm  = |b1 m| + c1 (A_gg + 2 |gg|) + |mm|
        c2 = 1 - b2;  vv = b2 v + c2 gg gg              A_vv  = |b2 v| + c2 gg^2 (3 + 2 A_gg / |gg|) + vv
        bc1 = 1 - b1^step                               A_bc1 = 2 POW_ULPS b1^step + bc1
        bc2 = 1 - b2^step;  rb = sqrt(bc2)              A_rb  = (2 POW_ULPS b2^step + bc2) / (2 rb) + rb
        sq = sqrt(vv)                                   A_sq  = A_vv / (2 sq) + sq
        den = sq / rb + eps                             A_den = A_sq / rb + sq A_rb / rb^2 + sq / rb + den
        a = lr / bc1;  r = mm / den                     A_a   = lr A_bc1 / bc1^2 + a;  A_r = A_mm / den + |mm| A_den / den^2 + |r|
        s = a r;  p' = p - s                            A_s   = A_a |r| + a A_r + |s|;  A_p = A_s + |p'|
        upd = p' - p                                    A_upd = A_p        (the kernel stores p' rounded: u |p'| is in upd too)

    A also holds "bc_rel" = A_bc1 / bc1 + A_rb / rb: the relative error the two bias corrections put on EVERY element of the
    update alike (at step 2, 1 - b2^2 = 0.002 keeps three digits less than b2^2), which a Frobenius bar of the update has to carry.

    fault: "bc2_nosqrt" the second bias correction without its square root; "scale_m_only" grad_scale on m but not on v."""
    bounds = bounds and dtype == torch.float64
    p, g, m, v = (_f(x, dtype).reshape(-1) for x in (p, g, m, v))
    lr, b1, b2, eps, gs = (torch.tensor(float(np.float32(x)), dtype=dtype) for x in (lr, b1, b2, eps, grad_scale))
    st = torch.tensor(float(step), dtype=dtype)
    gg = g * gs
    gv = g if fault == "scale_m_only" else gg
    c1, c2 = 1 - b1, 1 - b2
    mm = b1 * m + c1 * gg
    vv = b2 * v + c2 * gv * gv
    pw1, pw2 = torch.pow(b1, st), torch.pow(b2, st)
    bc1, bc2 = 1 - pw1, 1 - pw2
    rb = bc2 if fault == "bc2_nosqrt" else torch.sqrt(bc2)
    sq = torch.sqrt(vv)
    den = sq / rb + eps
    a = lr / bc1
    r = mm / den
    s = a * r
    pn = p - s
    out = {"m": mm, "v": vv, "p": pn, "upd": pn - p}
    if not bounds:
        return out, {}
    A_gg = gg.abs()
    A_mm = (b1 * m).abs() + c1 * (A_gg + 2 * gg.abs()) + mm.abs()
    A_vv = (b2 * v).abs() + c2 * gg * gg * 5 + vv
    A_bc1 = 2 * POW_ULPS * pw1 + bc1
    A_rb = (2 * POW_ULPS * pw2 + bc2) / (2 * rb) + rb
    A_sq = torch.where(sq > 0, A_vv / (2 * sq.clamp_min(1e-300)), torch.zeros_like(sq)) + sq
    A_den = A_sq / rb + sq * A_rb / rb ** 2 + sq / rb + den
    A_a = lr * A_bc1 / bc1 ** 2 + a
    A_r = A_mm / den + mm.abs() * A_den / den ** 2 + r.abs()
    A_s = A_a * r.abs() + a * A_r + s.abs()
    A_p = A_s + pn.abs()
    return out, {"m": A_mm, "v": A_vv, "p": A_p, "upd": A_p, "bc_rel": A_bc1 / bc1 + A_rb / rb}


def adam_upd_frob(ref, A):
    """Frobenius bar of the update: the step arithmetic at the bar of p (ADAM_FROB), the rounding of the stored p' (u |p'| per
    element, twice for the margin of C_BOUND) and the common relative error of the bias corrections, C_BOUND u bc_rel.

    How tight that is depends on the step.  bc_rel is dominated by 2 POW_ULPS b2^step / (2 bc2): about 2000 at step 1, 1000 at
    step 2 and 200 at step 10, so there the bar (and the per-element bound, which carries the same A_bc) is 2.5e-5 to 2.5e-4 of
    the update and a step mis-scaled by less than that passes -- although b^1 and 1 - b are exact at step 1.  This is the
    A_bc the bound is defined with.  Only at steps 1000 and 100000, where bc2 >= 0.63, is the update resolved to about 2.5e-6:
    the rows at those steps are the tight checks of the step size, the rows at steps 1, 2 and 10 check the rest (slices, the
    grid-stride pass, grad_scale, m and v)."""
    return ADAM_FROB + 2 * U * float(ref["p"].norm()) / (float(ref["upd"].norm()) + 1e-300) + C_BOUND * U * float(A["bc_rel"])


# ------------------------------------------------------------------------------------------------ integer kernels
def _order_key(logits):
    """float64 keys with the order of metrics_update: NaN above +inf above every finite value above -inf."""
    z = np.asarray(logits, dtype=np.float64)
    key = np.where(np.isposinf(z), 1e39, np.where(np.isneginf(z), -1e39, z))
    return np.where(np.isnan(z), 1e40, key)


def metrics_ref(logits, target, conf=None, conf2=None, fault=None):
    """metrics_update: pred = the first maximum over the classes (NaN counts as the maximum), second = the largest of the
    rest with the lowest index on ties, top2 = second where the target equals it, else pred; conf[t, pred] and
    conf2[t, top2] count the pixels with 0 <= t < K, added to the given matrices.  logits [B,K,...], target [B,...].
    fault: "transposed" conf[pred, t].  Returns (pred, top2, conf, conf2) as int64 numpy arrays."""
    z = np.asarray(torch.as_tensor(logits).detach().cpu().numpy())
    t = np.asarray(torch.as_tensor(target).detach().cpu().numpy()).astype(np.int64)
    B, K = z.shape[:2]
    key = np.moveaxis(_order_key(z).reshape(B, K, -1), 1, 2).reshape(-1, K)
    i1 = key.argmax(1)
    if K > 1:
        rest = key.copy()
        rest[np.arange(len(i1)), i1] = -1e41
        i2 = rest.argmax(1)
    else:
        i2 = np.zeros_like(i1)
    tf = t.reshape(-1)
    top2 = np.where(tf == i2, i2, i1)
    conf = np.zeros((K, K), np.int64) if conf is None else np.array(conf, dtype=np.int64)
    conf2 = np.zeros((K, K), np.int64) if conf2 is None else np.array(conf2, dtype=np.int64)
    ok = (tf >= 0) & (tf < K)
    if fault == "transposed":
        np.add.at(conf, (i1[ok], tf[ok]), 1)
    else:
        np.add.at(conf, (tf[ok], i1[ok]), 1)
    np.add.at(conf2, (tf[ok], top2[ok]), 1)
    return i1.reshape(t.shape), top2.reshape(t.shape), conf, conf2


def metrics_scan(logits, fault=None):
    """The same (pred, second) as a running scan over the classes, for the checker's own tests.  fault: "stale_second" the
    second maximum is not updated when the first is displaced."""
    z = np.asarray(torch.as_tensor(logits).detach().cpu().numpy())
    B, K = z.shape[:2]
    key = np.moveaxis(_order_key(z).reshape(B, K, -1), 1, 2).reshape(-1, K)
    v1, i1 = key[:, 0].copy(), np.zeros(len(key), np.int64)
    v2, i2 = np.full(len(key), -1e41), np.full(len(key), -1, np.int64)
    for k in range(1, K):
        v = key[:, k]
        first = v > v1
        second = ~first & ((i2 < 0) | (v > v2))
        if fault != "stale_second":
            v2, i2 = np.where(first, v1, v2), np.where(first, i1, i2)
        v2, i2 = np.where(second, v, v2), np.where(second, k, i2)
        v1, i1 = np.where(first, v, v1), np.where(first, k, i1)
    return i1, np.where(i2 < 0, 0, i2)


def confusion_add_ref(pred, target, K, conf=None):
    """confusion_add: conf[t, p] += 1 where both lie in [0, K)."""
    p = np.asarray(torch.as_tensor(pred).cpu().numpy()).reshape(-1).astype(np.int64)
    t = np.asarray(torch.as_tensor(target).cpu().numpy()).reshape(-1).astype(np.int64)
    conf = np.zeros((K, K), np.int64) if conf is None else np.array(conf, dtype=np.int64)
    ok = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    np.add.at(conf, (t[ok], p[ok]), 1)
    return conf


def _differs(y):
    """[B,H,W] bool: a 4-neighbour inside the image holds another label."""
    y = np.asarray(torch.as_tensor(y).cpu().numpy()).astype(np.int64)
    d = np.zeros(y.shape, bool)
    d[:, 1:] |= y[:, 1:] != y[:, :-1]
    d[:, :-1] |= y[:, :-1] != y[:, 1:]
    d[:, :, 1:] |= y[:, :, 1:] != y[:, :, :-1]
    d[:, :, :-1] |= y[:, :, :-1] != y[:, :, 1:]
    return y, d


def boundary_target_ref(y):
    return _differs(y)[1].astype(np.int64)


def region_relabel_ref(y, keep_boundary, ignore_label):
    y, d = _differs(y)
    return np.where(d == bool(keep_boundary), y, np.int64(ignore_label))


# ------------------------------------------------------------------------------------------------ inputs of the rows
def make_loss_inputs(row):
    """Logits [B,K,H,W] float32, targets [B,H,W] int64 and class weights [K] float32 | None of a row of the loss tables.

    logits:  "normal" | "x8" | "+80" | "-80" | "ties" (integers: exact ties) | "sat" (every second pixel: the target logit 25
             above the largest other one, so that pt == 1.f in float32)
    ignore:  the ignore_index (a fifth of the pixels take it; inside [0, K) it is simply that class)
    bad:     labels K and -7 at a few pixels        ignore_block: pixels 256..511 all ignored      all_ignored
    weights: None | "rand0" (random, one class at 0) | "zero_block" (rand0, and pixels 256..511 all on the zero-weight class)"""
    B, K, H, W = row["B"], row["K"], row["H"], row["W"]
    gen = torch.Generator().manual_seed(row["seed"])
    z = torch.randn(B, K, H, W, generator=gen)
    kind = row.get("logits", "normal")
    t = torch.randint(0, K, (B, H, W), generator=gen)
    if kind == "x8":
        z = z * 8
    elif kind in ("+80", "-80"):
        z = z + float(kind)
    elif kind == "ties":
        z = torch.round(z)
    ign = row.get("ignore", -100)
    tf = t.reshape(-1)
    n = tf.numel()
    drop = torch.rand(n, generator=gen) < 0.2
    if row.get("all_ignored"):
        drop[:] = True
    if ign is not None:                                   # None: the loss has no ignore_index (smooth CE)
        tf[drop] = ign
    zero = K - 1                                          # the class whose weight is 0 when the row has weights
    if not row.get("all_ignored"):                        # at least one kept pixel with a positive weight
        live = [c for c in range(K) if c != ign and not (row.get("weights") and K > 1 and c == zero)]
        assert live, "the row leaves no class that is kept and weighted"
        tf[min(1, n - 1)] = live[0]
    if row.get("ignore_block"):
        assert n >= 512
        tf[256:512] = ign
    cw = None
    if row.get("weights"):
        cw = torch.rand(K, generator=gen) + 0.5
        if K > 1:
            cw[zero] = 0.0
        if row["weights"] == "zero_block":
            assert n >= 512 and K > 1
            tf[256:512] = zero
    if row.get("bad"):
        for i, val in zip((0, n // 3, n // 2 + 1, n - 1) if n >= 8 else (0,), (K, -7, K, -7)):
            tf[i] = val
    if kind == "sat":
        zr = z.reshape(B, K, -1).permute(0, 2, 1).reshape(-1, K)
        for i in range(0, n, 2):
            c = int(tf[i])
            if 0 <= c < K:
                other = torch.cat([zr[i, :c], zr[i, c + 1:]])
                zr[i, c] = (float(other.max()) if K > 1 else 0.0) + 25.0
        z = zr.reshape(B, -1, K).permute(0, 2, 1).reshape(B, K, H, W).contiguous()
    return z.contiguous(), tf.reshape(B, H, W), cw


def saturated(logits, target):
    """bool [B*H*W]: pixels whose pt is exactly 1.f in a float32 evaluation (valid targets only)."""
    K = logits.shape[1]
    z = _rows(logits, torch.float32)
    t = torch.as_tensor(target).reshape(-1).long()
    ok = (t >= 0) & (t < K)
    mx = z.max(1, keepdim=True).values
    s = torch.exp(z - mx).sum(1)
    lpt = (z - mx).gather(1, t.clamp(0, K - 1)[:, None])[:, 0] - torch.log(s)
    return ok & (torch.exp(lpt) == 1.0)


def make_adam_inputs(row):
    """(buf_p, buf_g, buf_m, buf_v, offset, n): four float32 buffers of offset + n + 5 elements; the step runs on
    [offset, offset + n) and the elements around it must stay untouched.  grad: "normal" | "zero" (zero state too) | "tiny"
    (1e-30, p = 0) | "huge" (1e15)."""
    n, off = row["n"], row.get("offset", 0)
    gen = torch.Generator().manual_seed(row["seed"])
    tot = off + n + 5
    p = torch.randn(tot, generator=gen) * 1e-2
    g = torch.randn(tot, generator=gen)
    m = torch.randn(tot, generator=gen) * 0.1
    v = torch.rand(tot, generator=gen) * 0.01
    kind = row.get("grad", "normal")
    if kind == "zero":
        g, m, v = torch.zeros(tot), torch.zeros(tot), torch.zeros(tot)
    elif kind == "tiny":
        g = torch.full((tot,), 1e-30) * torch.sign(g)
        p, m, v = torch.zeros(tot), torch.zeros(tot), torch.zeros(tot)
    elif kind == "huge":
        g = g * 1e15
        m, v = m * 1e15, v * 1e30
    return p, g, m, v, off, n
