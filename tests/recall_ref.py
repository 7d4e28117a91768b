"""Independent float64 reference of RecallCrossEntropy (csrc/loss.hip) with per-element error bounds (CPU only), in the
conventions of tests/tail_ref.py: explicit formulas, forward and backward, each line next to its bound; a kernel result must
satisfy |got - ref64| <= C_BOUND * u * A + 1e-30 element by element, with tail_ref's C_BOUND = 2 and EXP_ULPS = LOG_ULPS = 2 and
no constant of its own.  The softmax pieces, the total of the pixel terms and the comparison are tail_ref's (_softmax, _total,
assert_within).

The rule (logits z [B,K,H,W], target t [B,H,W], N = B*H*W counts every pixel; a pixel is valid when t lies in [0, K) and is
not ignore_index):

    pred = first maximum over the classes, NaN counting as the maximum (tail_ref._order_key: metrics_update's rule)
    gt_c = #{valid, t = c};  fn_c = #{valid, t = c, pred != c}          numpy integers, compared bit for bit
    w_c  = float32(float64(max(fn_c, 1)) / float64(max(gt_c, 1)))        one rounding, the same in the kernel: exact data

        nll = lse - z_t                                 A_nll = A_lse + |nll|
        l = w_t nll                                     A_l   = w_t A_nll + |l|
        num = sum_valid l                               _total()
        loss = num / N (+ prior)                        A     = A_num / N + |loss| (+ |prior| + |sum|)
        rn = 1 / N                                      A_rn  = rn            (rounded once to float)
        c = w_t rn                                      A_c   = w_t A_rn + c
        g_k = c (p_k - [k=t])                           A_g   = A_c |p - 1| + c (A_p + |p - 1|) + |g|

Planted faults (for the checker's own tests): "fn_all" fn counts every pixel of the class; "no_floor" weight 0 at perfect
recall; "mean_valid" the sum divided by the number of valid pixels; "argmax_last" the last maximum on ties; "partial" the 256
pixels from 131072 on (the second grid pass) missing from the total.

Nothing here imports crop2seg_amd or oracle.
"""
import numpy as np
import torch

from tail_ref import (C_BOUND, EXP_ULPS, LOG_ULPS, U, _f, _nchw, _order_key, _rows, _softmax, _total,  # noqa: F401
                      assert_within, bound_ratio)

GRID_PIXELS = 512 * 256        # pixels of one grid pass of recall_count / recall_loss / recall_bwd


def recall_counts(logits, target, ignore_index, fault=None):
    """(pred [N], valid [N], gt [K], fn [K], bad, w [K] float32) from integers alone."""
    z = np.asarray(torch.as_tensor(logits).detach().cpu().numpy())
    B, K = z.shape[:2]
    key = np.moveaxis(_order_key(z).reshape(B, K, -1), 1, 2).reshape(-1, K)
    pred = K - 1 - key[:, ::-1].argmax(1) if fault == "argmax_last" else key.argmax(1)
    t = np.asarray(torch.as_tensor(target).detach().cpu().numpy()).astype(np.int64).reshape(-1)
    inside = (t >= 0) & (t < K)
    valid = inside & (t != ignore_index)
    bad = int((~inside & (t != ignore_index)).sum())
    gt = np.bincount(t[valid], minlength=K).astype(np.int64)
    fn = gt.copy() if fault == "fn_all" else np.bincount(t[valid & (pred != t)], minlength=K).astype(np.int64)
    F = fn if fault == "no_floor" else np.maximum(fn, 1)
    w = (F.astype(np.float64) / np.maximum(gt, 1).astype(np.float64)).astype(np.float32)
    return pred, valid, gt, fn, bad, w


def recall_ref(logits, target, ignore_index=255, prior=None, dtype=torch.float64, bounds=True, fault=None):
    """Returns ({loss [1], glogits [B,K,H,W], nll [N] (0 where not valid), tot [1] (the sum of w_t nll), weights [K] float32,
    counts [2,K] int64, bad int}, {bounds of loss, glogits, nll, tot})."""
    bounds = bounds and dtype == torch.float64
    shape = tuple(logits.shape)
    K = shape[1]
    z = _rows(logits, dtype)
    N = z.shape[0]
    _, valid, gt, fn, bad, w32 = recall_counts(logits, target, ignore_index, fault)
    keep = torch.from_numpy(valid)
    t = torch.as_tensor(target).reshape(-1).long().cpu()
    y = t.clamp(0, K - 1)
    w = torch.from_numpy(w32).to(dtype)
    o, A = _softmax(z, bounds)
    onehot = torch.zeros_like(z).scatter_(1, y[:, None], 1.0)
    zero = torch.zeros(N, dtype=dtype)
    nll = torch.where(keep, (o["lse"] - z).gather(1, y[:, None])[:, 0], zero)
    wt = w[y]
    l = torch.where(keep, wt * nll, zero)
    inc = torch.ones_like(l)
    if fault == "partial":
        inc[GRID_PIXELS:GRID_PIXELS + 256] = 0
    num = (l * inc).sum()
    div = float(max(int(valid.sum()), 1)) if fault == "mean_valid" else float(N)
    mean = num / div
    loss = mean if prior is None else _f(prior, dtype).reshape(()) + mean
    rn = torch.tensor(1.0 / N, dtype=dtype)
    c = wt * rn
    pm = o["p"] - onehot
    g = torch.where(keep[:, None], c[:, None] * pm, torch.zeros_like(pm))
    out = {"loss": loss.reshape(1), "glogits": _nchw(g, shape), "nll": nll, "tot": num.reshape(1),
           "weights": w32, "counts": np.stack([gt, fn]), "bad": bad}
    if not bounds:
        return out, {}
    A_nll = torch.where(keep, A["lse"][:, 0] + nll.abs(), zero)
    A_l = torch.where(keep, wt * A_nll + l.abs(), zero)
    _, A_num = _total(l, A_l)
    A_mean = A_num / N + mean.abs()
    A_loss = A_mean if prior is None else A_mean + _f(prior, dtype).abs().reshape(()) + loss.abs()
    A_rn = rn
    A_c = wt * A_rn + c
    A_g = A_c[:, None] * pm.abs() + c[:, None] * (A["p"] + pm.abs()) + g.abs()
    A_g = torch.where(keep[:, None], A_g, torch.zeros_like(A_g))
    return out, {"loss": A_loss.reshape(1), "glogits": _nchw(A_g, shape), "nll": A_nll, "tot": (A_num + num.abs()).reshape(1)}
