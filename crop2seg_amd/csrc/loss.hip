// The four criteria on [B,K,H,W] logits: cross entropy, focal CE, smooth CE and recall CE.  Each is a forward kernel that
// leaves float block partials in a fixed order, a one-thread finalize kernel that sums them in double, and a backward kernel
// (smooth CE: one pass for both).  What they share is stated once, below; the loss and gradient expressions are each kernel's.
// No float atomics: loss and gradient are bitwise reproducible from run to run.  Everything is stream-ordered.
#include "common.h"

namespace {

constexpr int MAXK = C2S_MAX_CLASSES;     // smooth CE (a 32-bit class mask) and recall CE (registers, LDS histograms)
constexpr int LOSS_BLOCKS = 512;          // grid cap of every forward kernel: the partial count fixes the bits of the loss

// A target outside [0, K) that is not ignore_index makes torch raise (device assert); here it is skipped like
// ignore_index -- no out-of-bounds read -- and counted ("bad").
__device__ __forceinline__ bool valid_target(long long t, int K, long long ignore_index) {
    return !(t == ignore_index || t < 0 || t >= K);
}

// element e of [B, HW] -> offset of its class-0 value in [B, K, HW]; class k follows at k * HW
__device__ __forceinline__ size_t pixel_offset(long e, int K, int HW) {
    const int pix = (int)(e % HW), b = (int)(e / HW);
    return (size_t)b * K * HW + pix;
}

__device__ __forceinline__ void zero_row(float* __restrict__ gp, int K, int HW) {
    for (int k = 0; k < K; ++k) gp[(size_t)k * HW] = 0.f;
}

// mx = max_k z_k, s = sum_k exp(z_k - mx), in class order.  FAST: __expf (cross entropy) or expf (focal, smooth CE)
template <bool FAST>
__device__ __forceinline__ void softmax_stats(const float* __restrict__ lp, int K, int HW, float& mx, float& s) {
    mx = lp[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, lp[(size_t)k * HW]);
    s = 0.f;
    for (int k = 0; k < K; ++k) s += FAST ? __expf(lp[(size_t)k * HW] - mx) : expf(lp[(size_t)k * HW] - mx);
}

// part[block * N + j] = the block's sum of v[j] (256 threads): wave sums, then (w0 + w1) + (w2 + w3)
template <int N>
__device__ __forceinline__ void block_partials(float (&v)[N], float* __restrict__ part) {
    __shared__ float red[4][N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = wave_sum(v[j]);
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < N; ++j) red[threadIdx.x >> 6][j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < N; ++j) part[blockIdx.x * N + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
}

// the finalize kernels: one thread adds the partials to acc (zeros) serially in double, then writes the loss or adds to it
template <int N>
__device__ __forceinline__ void sum_partials(const float* __restrict__ part, int blocks, double (&acc)[N]) {
    for (int i = 0; i < blocks; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] += part[i * N + j];
    }
}
__device__ __forceinline__ void store_loss(float* __restrict__ loss, float l, int accumulate) {
    *loss = accumulate ? *loss + l : l;
}

// ---------------------------------------------------------------- cross entropy (train.py:463-468)
// nn.CrossEntropyLoss(weight=w, label_smoothing=eps), reduction "mean" (torch semantics with class weights):
//   loss_i = (1-eps) w[y_i] (-log p_i[y_i]) + (eps/K) sum_k w[k] (-log p_i[k]);  loss = sum_i loss_i / sum_i w[y_i]
// Pixels whose target equals ignore_index (torch default -100) contribute to neither sum.
// per block partial (sum loss_i, sum w, bad) -> ws[3*blocks]; finalize -> ws_tot[3]; grad kernel uses ws_tot[1]
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ cw, float* __restrict__ part, int B, int K,
                                                     int HW, float eps, long long ignore_index) {
    const long total = (long)B * HW;
    float num = 0.f, den = 0.f, bad = 0.f;
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long long yy = target[e];
        if (!valid_target(yy, K, ignore_index)) { bad += yy != ignore_index ? 1.f : 0.f; continue; }
        const int y = (int)yy;
        const float* lp = logits + pixel_offset(e, K, HW);
        float mx, s;
        softmax_stats<true>(lp, K, HW, mx, s);
        const float w = cw[y];
        const float lse = mx + __logf(s);
        float li = w * (lse - lp[(size_t)y * HW]);
        if (eps > 0.f) {
            float sm = 0.f;
            for (int k = 0; k < K; ++k) sm += cw[k] * (lse - lp[(size_t)k * HW]);
            li = (1.f - eps) * li + (eps / (float)K) * sm;
        }
        num += li;
        den += w;
    }
    float v[3] = {num, den, bad};
    block_partials(v, part);
}

__global__ void ce_finalize_kernel(const float* __restrict__ part, float* __restrict__ tot, float* __restrict__ loss,
                                   int blocks) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a[3] = {};                                   // num, den, bad
    sum_partials(part, blocks, a);
    tot[0] = (float)a[0]; tot[1] = (float)a[1]; tot[2] = (float)a[2];
    store_loss(loss, (float)(a[0] / a[1]), 0);
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ cw, const float* __restrict__ tot,
                                                     float* __restrict__ glogits, int B, int K, int HW, float eps,
                                                     long long ignore_index) {
    const long total = (long)B * HW;
    const float inv_den = 1.f / tot[1];
    float wsum = 0.f;
    if (eps > 0.f)
        for (int k = 0; k < K; ++k) wsum += cw[k];
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const float* lp = logits + pixel_offset(e, K, HW);
        float* gp = glogits + pixel_offset(e, K, HW);
        const long long yy = target[e];
        if (!valid_target(yy, K, ignore_index)) { zero_row(gp, K, HW); continue; }
        const int y = (int)yy;
        float mx, s;
        softmax_stats<true>(lp, K, HW, mx, s);
        const float w = cw[y] * inv_den, inv_s = 1.f / s;
        if (eps > 0.f) {
            // (1-eps) w_y (p_k - delta_ky) + (eps/K) (W p_k - w_k), all over sum_i w[y_i]
            const float a = (1.f - eps) * w, c = eps / (float)K * inv_den;
            for (int k = 0; k < K; ++k) {
                const float pk = __expf(lp[(size_t)k * HW] - mx) * inv_s;
                gp[(size_t)k * HW] = a * (pk - (k == y ? 1.f : 0.f)) + c * (wsum * pk - cw[k]);
            }
        } else {
            for (int k = 0; k < K; ++k)
                gp[(size_t)k * HW] = w * (__expf(lp[(size_t)k * HW] - mx) * inv_s - (k == y ? 1.f : 0.f));
        }
    }
}

// ---------------------------------------------------------------- focal CE
// FocalCELoss (focal_loss.py:12-45): part[block] = (sum over kept pixels of f = -(1-pt)^g log pt, #kept, sum of w[target]).
// With class weights the reference multiplies a [N,1] column of weights by the [N] row of focal terms (focal_loss.py:36-39:
// `w.gather(1, target)` keeps the column shape) -- an N x N outer product, so its value is
//   size_average: mean_i(w_i) * mean_j(f_j),   else: sum_i(w_i) * sum_j(f_j)
// and that is what is computed here (without the N^2 tensor, which is 17 GB at B=4, 128x128); pinned by fixtures written from
// the imported module (oracle/make_golden_tail.py).  d/dz: the weights do not depend on the logits -- a constant factor.
__global__ __launch_bounds__(256) void focal_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                        const float* __restrict__ class_w, float* __restrict__ part, int B, int K,
                                                        int HW, float gamma, long long ignore_index) {
    const long total = (long)B * HW;
    float num = 0.f, cnt = 0.f, wsum = 0.f;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long long t = target[e];
        if (!valid_target(t, K, ignore_index)) continue;
        const float* lp = logits + pixel_offset(e, K, HW);
        float mx, s;
        softmax_stats<false>(lp, K, HW, mx, s);
        const float logpt = lp[(size_t)t * HW] - mx - logf(s);
        const float pt = expf(logpt);
        num += -powf(1.f - pt, gamma) * logpt;
        cnt += 1.f;
        wsum += class_w ? class_w[t] : 1.f;
    }
    float v[3] = {num, cnt, wsum};
    block_partials(v, part);
}

// tot = (sum f, #kept, d loss / d (sum f))
__global__ void focal_finalize_kernel(const float* __restrict__ part, float* __restrict__ tot, float* __restrict__ loss,
                                      int blocks, int weighted, int size_average, int accumulate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a[3] = {};
    sum_partials(part, blocks, a);
    const double num = a[0], cnt = a[1], wsum = a[2];
    const double scale = weighted ? (size_average ? wsum / (cnt * cnt) : wsum) : (size_average ? 1.0 / cnt : 1.0);
    tot[0] = (float)num; tot[1] = (float)cnt; tot[2] = (float)scale;
    store_loss(loss, (float)(num * scale), accumulate);
}

// d/dz_k of -(1-pt)^g log pt = [g (1-pt)^(g-1) pt log pt - (1-pt)^g] (delta_kt - p_k)
__global__ __launch_bounds__(256) void focal_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                        const float* __restrict__ tot, float* __restrict__ glogits, int B,
                                                        int K, int HW, float gamma, long long ignore_index) {
    const long total = (long)B * HW;
    const float inv_n = tot[2];
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const float* lp = logits + pixel_offset(e, K, HW);
        float* gp = glogits + pixel_offset(e, K, HW);
        const long long t = target[e];
        if (!valid_target(t, K, ignore_index)) { zero_row(gp, K, HW); continue; }
        float mx, s;
        softmax_stats<false>(lp, K, HW, mx, s);
        const float inv_s = 1.f / s;
        const float logpt = lp[(size_t)t * HW] - mx - logf(s);
        const float pt = expf(logpt);
        const float om = 1.f - pt;
        // dL/dlogpt = g (1-pt)^(g-1) pt logpt - (1-pt)^g ; dlogpt/dz_k = delta_kt - p_k
        // At a saturated pixel (pt == 1.f: om == 0, logpt == 0) om^(g-1) is inf for every g < 1 and the first term inf * 0; its
        // limit is finite (logpt ~ -om, so the term goes like -g om^g -> 0), and for g == 0 the loss is plain CE: the term is 0.
        // The factor is taken as 0 there, so no inf is formed; elsewhere the expression is the one above.
        const bool at_limit = gamma < 1.f && (gamma == 0.f || om <= 0.f);
        const float om_gm1 = at_limit ? 0.f : powf(om, gamma - 1.f);
        const float coef = (gamma * om_gm1 * pt * logpt - powf(om, gamma)) * inv_n;
        for (int k = 0; k < K; ++k) {
            const float pk = expf(lp[(size_t)k * HW] - mx) * inv_s;
            gp[(size_t)k * HW] = coef * ((k == t ? 1.f : 0.f) - pk);
        }
    }
}

// ---------------------------------------------------------------- smooth CE
// SmoothCrossEntropy2D (smooth_loss.py:58-84): soft targets from the 4-neighbourhood dilation of the label map -- the classes
// present at a pixel or its 4 neighbours (zero padding) share 1 - eps*(K - n) evenly, every other class gets eps = ls/K;
// pixels labelled `bg_index` take the fixed distribution `bg` instead (background_treatment) -- then CrossEntropyLoss with
// probability targets: mean over ALL B*H*W pixels of -sum_k w_k t_k log_softmax(z)_k.  One pass: the class set of a pixel is
// a bit mask built from five labels (no one-hot tensor, no depthwise convolution), the loss term and d/dz of the pixel come
// from the same softmax.  part[block] = (sum of pixel losses, labels outside [0,K) seen -- the reference's one_hot raises
// on those; here they are counted and the pixel contributes nothing).
__global__ __launch_bounds__(256) void smooth_ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                        const float* __restrict__ class_w, const float* __restrict__ bg,
                                                        float* __restrict__ part, float* __restrict__ glogits,
                                                        float* __restrict__ pixel_loss, int B, int K, int H, int W, float ls,
                                                        long long bg_index, float inv_n) {
    const int HW = H * W;
    const long total = (long)B * HW;
    const float eps = ls / (float)K;
    float num = 0.f, bad = 0.f;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int pix = (int)(e % HW), x = pix % W, r = pix / W;
        const float* lp = logits + pixel_offset(e, K, HW);
        float* gp = glogits ? glogits + pixel_offset(e, K, HW) : nullptr;
        const long long t = target[e];
        if (t < 0 || t >= K) {
            bad += 1.f;
            if (gp) zero_row(gp, K, HW);
            if (pixel_loss) pixel_loss[e] = 0.f;
            continue;
        }
        unsigned mask = 1u << (int)t;
        if (r > 0) { const long long v = target[e - W]; if (v >= 0 && v < K) mask |= 1u << (int)v; }
        if (r < H - 1) { const long long v = target[e + W]; if (v >= 0 && v < K) mask |= 1u << (int)v; }
        if (x > 0) { const long long v = target[e - 1]; if (v >= 0 && v < K) mask |= 1u << (int)v; }
        if (x < W - 1) { const long long v = target[e + 1]; if (v >= 0 && v < K) mask |= 1u << (int)v; }
        const float nd = (float)__popc(mask);
        const float exp_small = eps * ((float)K - nd);
        const float exp_large = (1.f - exp_small) / nd;
        const bool is_bg = bg != nullptr && t == bg_index;
        float mx, s;
        softmax_stats<false>(lp, K, HW, mx, s);
        const float lse = mx + logf(s);
        const float inv_s = 1.f / s;
        float loss = 0.f, wsum = 0.f;
        for (int k = 0; k < K; ++k) {
            const float tk = is_bg ? bg[k] : (((mask >> k) & 1u) ? exp_large : eps);
            const float wt = (class_w ? class_w[k] : 1.f) * tk;
            loss -= wt * (lp[(size_t)k * HW] - lse);
            wsum += wt;
        }
        num += loss;
        if (pixel_loss) pixel_loss[e] = loss;
        if (gp) {
            for (int k = 0; k < K; ++k) {
                const float tk = is_bg ? bg[k] : (((mask >> k) & 1u) ? exp_large : eps);
                const float wt = (class_w ? class_w[k] : 1.f) * tk;
                const float pk = expf(lp[(size_t)k * HW] - mx) * inv_s;
                gp[(size_t)k * HW] = (pk * wsum - wt) * inv_n;
            }
        }
    }
    float v[2] = {num, bad};
    block_partials(v, part);
}

__global__ void smooth_ce_finalize_kernel(const float* __restrict__ part, float* __restrict__ tot, float* __restrict__ loss,
                                          int blocks, double npix, int accumulate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a[2] = {};                                   // num, bad
    sum_partials(part, blocks, a);
    tot[0] = (float)a[0]; tot[1] = (float)a[1];
    store_loss(loss, (float)(a[0] / npix), accumulate);
}

// ---------------------------------------------------------------- recall CE (arXiv 2106.14917)
// Cross entropy weighted per class by the batch's false-negative share,
//   pred = argmax_k z_k (first maximum, NaN counts as the maximum: metrics_update_kernel's rule == torch.argmax)
//   gt_c = #{valid pixels with t = c},  fn_c = #{valid pixels with t = c and pred != c}
//   w_c  = max(fn_c, 1) / max(gt_c, 1)            (the reference's counters start from torch.ones, :28,37)
//   loss = (1 / N) sum_valid w_t (lse(z) - z_t),   N = B*H*W: ALL pixels (the reference's .mean() of a reduction='none' tensor)
//   dL/dz_k = (w_t / N) (p_k - [k = t]) on valid pixels, 0 elsewhere: the weights come from an argmax and are constants.
// The weights need a reduction over the whole batch before any pixel's term is known, so the pass is split:
//   recall_zero_kernel     zeroes the counters (a kernel, not a memset: a replayed hipGraph zeroes them again)
//   recall_count_kernel    the first read of the logits: argmax, nll per pixel -> workspace, LDS histograms gt / fn / bad,
//                          one 64-bit integer atomic per non-zero bin (order independent, bit-exact)
//   recall_weights_kernel  w_c, published with the counts
//   recall_loss_kernel     float block partials of w_t nll; recall_finalize_kernel in double
//   recall_bwd_kernel      the second and last read of the logits
// The two kernels that read the logits keep their register form (load_pixel) and their own statistics: an argmax with the
// NaN rule and a log-sum-exp around the arg-max value are not softmax_stats.
constexpr int NCOUNT = 2 * MAXK + 1;      // gt[MAXK], fn[MAXK], bad

// Workspace (floats), n = B*HW:
//   [0, n) nll | [n, n + LOSS_BLOCKS) block partials | NCOUNT 64-bit counters in 2*NCOUNT + 1 floats (one float of slack:
//   the counters start at the first 8-byte boundary) | w[MAXK] | (sum of w_t nll, bad-label count)
inline size_t recall_ws_floats(long n) { return (size_t)n + LOSS_BLOCKS + (2 * NCOUNT + 1) + MAXK + 2; }

__global__ void recall_zero_kernel(unsigned long long* __restrict__ cnt) {
    for (int i = threadIdx.x; i < NCOUNT; i += blockDim.x) cnt[i] = 0ull;
}

// The K logits of a pixel, read once into registers (the loops are unrolled to MAXK, K is uniform).
__device__ __forceinline__ void load_pixel(const float* __restrict__ lp, int K, int HW, float (&v)[MAXK]) {
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
        if (k < K) v[k] = lp[(size_t)k * HW];
}

__global__ __launch_bounds__(256) void recall_count_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                           float* __restrict__ nll, unsigned long long* __restrict__ cnt, int B,
                                                           int K, int HW, long long ignore_index) {
    __shared__ unsigned int h[NCOUNT];
    for (int i = threadIdx.x; i < NCOUNT; i += 256) h[i] = 0;
    __syncthreads();
    const long total = (long)B * HW;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long long t = target[e];
        if (!valid_target(t, K, ignore_index)) {
            if (t != ignore_index) atomicAdd(&h[2 * MAXK], 1u);
            nll[e] = 0.f;
            continue;
        }
        float v[MAXK];
        load_pixel(logits + pixel_offset(e, K, HW), K, HW, v);
        float v1 = v[0], zt = v[0];
        int i1 = 0;
#pragma unroll
        for (int k = 1; k < MAXK; ++k) {
            if (k < K) {
                if (v[k] > v1 || (v[k] != v[k] && v1 == v1)) { v1 = v[k]; i1 = k; }   // NaN counts as the maximum
                if (k == (int)t) zt = v[k];
            }
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) s += expf(v[k] - v1);
        nll[e] = (v1 + logf(s)) - zt;
        atomicAdd(&h[(int)t], 1u);
        if (i1 != (int)t) atomicAdd(&h[MAXK + (int)t], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NCOUNT; i += 256)
        if (h[i]) atomicAdd(cnt + i, (unsigned long long)h[i]);
}

// w_c = (float)((double)max(fn_c, 1) / (double)max(gt_c, 1)); counts_out [2][K] = (gt, fn) before the floor
__global__ void recall_weights_kernel(const unsigned long long* __restrict__ cnt, float* __restrict__ w, float* __restrict__ tot,
                                      float* __restrict__ weights_out, long long* __restrict__ counts_out, int K) {
    const int k = threadIdx.x;
    if (k < K) {
        const unsigned long long gt = cnt[k], fn = cnt[MAXK + k];
        const float wk = (float)((double)(fn > 0 ? fn : 1ull) / (double)(gt > 0 ? gt : 1ull));
        w[k] = wk;
        if (weights_out) weights_out[k] = wk;
        if (counts_out) { counts_out[k] = (long long)gt; counts_out[K + k] = (long long)fn; }
    }
    if (k == 0) tot[1] = (float)cnt[2 * MAXK];
}

__global__ __launch_bounds__(256) void recall_loss_kernel(const float* __restrict__ nll, const int64_t* __restrict__ target,
                                                          const float* __restrict__ w, float* __restrict__ part, long total,
                                                          int K, long long ignore_index) {
    __shared__ float ws[MAXK];
    if (threadIdx.x < K) ws[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    float num = 0.f;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long long t = target[e];
        if (!valid_target(t, K, ignore_index)) continue;
        num += ws[(int)t] * nll[e];
    }
    float v[1] = {num};
    block_partials(v, part);
}

__global__ void recall_finalize_kernel(const float* __restrict__ part, float* __restrict__ tot, float* __restrict__ loss,
                                       int blocks, double npix, int accumulate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a[1] = {};
    sum_partials(part, blocks, a);
    tot[0] = (float)a[0];                               // tot[1], the bad-label count, is recall_weights_kernel's
    store_loss(loss, (float)(a[0] / npix), accumulate);
}

__global__ __launch_bounds__(256) void recall_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                         const float* __restrict__ w, float* __restrict__ glogits, int B, int K,
                                                         int HW, long long ignore_index, float inv_n) {
    __shared__ float ws[MAXK];
    if (threadIdx.x < K) ws[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const long total = (long)B * HW;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        float* gp = glogits + pixel_offset(e, K, HW);
        const long long t = target[e];
        if (!valid_target(t, K, ignore_index)) { zero_row(gp, K, HW); continue; }
        float v[MAXK];
        load_pixel(logits + pixel_offset(e, K, HW), K, HW, v);
        float mx = v[0];
#pragma unroll
        for (int k = 1; k < MAXK; ++k)
            if (k < K) mx = fmaxf(mx, v[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) { v[k] = expf(v[k] - mx); s += v[k]; }
        const float inv_s = 1.f / s, c = ws[(int)t] * inv_n;
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
            if (k < K) gp[(size_t)k * HW] = c * (v[k] * inv_s - (k == (int)t ? 1.f : 0.f));
    }
}

}  // namespace

extern "C" size_t c2s_cross_entropy_workspace_floats(int, int) { return 3 * LOSS_BLOCKS + 3; }

extern "C" int c2s_cross_entropy(const float* logits, const int64_t* target, const float* class_w, float* loss,
                                 float* glogits, int B, int K, int HW, float label_smoothing, long long ignore_index,
                                 float* workspace, size_t ws_floats, void* stream) {
    C2S_REQUIRE(logits && target && class_w && loss && workspace, "cross_entropy: null pointer");
    C2S_REQUIRE(ws_floats >= 3 * LOSS_BLOCKS + 3 && B > 0 && K > 0 && HW > 0, "cross_entropy: bad args");
    C2S_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "cross_entropy: label_smoothing must be in [0, 1]");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid_for((long)B * HW, LOSS_BLOCKS);
    float* tot = workspace + 3 * LOSS_BLOCKS;    // (sum, weight sum, targets outside [0,K) other than ignore_index)
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(blocks), dim3(256), 0, st, logits, target, class_w, workspace, B, K, HW,
                       label_smoothing, ignore_index);
    C2S_CHECK_LAUNCH("ce_fwd");
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(64), 0, st, workspace, tot, loss, blocks);
    C2S_CHECK_LAUNCH("ce_finalize");
    if (glogits != nullptr) {
        hipLaunchKernelGGL(ce_bwd_kernel, dim3(blocks), dim3(256), 0, st, logits, target, class_w, tot, glogits, B, K, HW,
                           label_smoothing, ignore_index);
        C2S_CHECK_LAUNCH("ce_bwd");
    }
    return C2S_OK;
}

extern "C" size_t c2s_focal_ce_workspace_floats(void) { return 3 * LOSS_BLOCKS + 4; }

extern "C" int c2s_focal_ce_ex(const float* logits, const long long* target, const float* class_w, float* loss, float* glogits,
                               int B, int K, int HW, float gamma, long long ignore_index, int size_average, int accumulate_loss,
                               float* workspace, size_t ws_floats, void* stream) {
    C2S_REQUIRE(logits && target && loss && workspace, "focal_ce: null pointer");
    C2S_REQUIRE(B > 0 && K > 0 && HW > 0 && gamma >= 0.f, "focal_ce: bad args");
    C2S_REQUIRE(ws_floats >= c2s_focal_ce_workspace_floats(), "focal_ce: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid_for((long)B * HW, LOSS_BLOCKS);
    float* tot = workspace + 3 * LOSS_BLOCKS;
    hipLaunchKernelGGL(focal_fwd_kernel, dim3(blocks), dim3(256), 0, st, logits, (const int64_t*)target, class_w, workspace, B, K,
                       HW, gamma, ignore_index);
    C2S_CHECK_LAUNCH("focal_fwd");
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(64), 0, st, workspace, tot, loss, blocks, class_w != nullptr ? 1 : 0,
                       size_average, accumulate_loss);
    C2S_CHECK_LAUNCH("focal_finalize");
    if (glogits) {
        hipLaunchKernelGGL(focal_bwd_kernel, dim3(grid_for((long)B * HW, 2048)), dim3(256), 0, st, logits, (const int64_t*)target, tot,
                           glogits, B, K, HW, gamma, ignore_index);     // no partials here: the grid is wider than the forward's
        C2S_CHECK_LAUNCH("focal_bwd");
    }
    return C2S_OK;
}

extern "C" int c2s_focal_ce(const float* logits, const long long* target, float* loss, float* glogits, int B, int K, int HW,
                            float gamma, long long ignore_index, int accumulate_loss, float* workspace, size_t ws_floats,
                            void* stream) {
    return c2s_focal_ce_ex(logits, target, nullptr, loss, glogits, B, K, HW, gamma, ignore_index, 1, accumulate_loss, workspace,
                           ws_floats, stream);
}

extern "C" size_t c2s_smooth_ce_workspace_floats(void) { return 2 * LOSS_BLOCKS + 2; }

// reduction: 0 'mean' (over all B*H*W pixels), 1 'sum', 2 'none' (pixel_loss [B,H,W] receives the per-pixel terms; *loss their
// sum and glogits the gradient of that sum)
extern "C" int c2s_smooth_ce_ex(const float* logits, const long long* target, const float* class_w, const float* bg_distrib,
                                float* loss, float* glogits, float* pixel_loss, int B, int K, int H, int W, float label_smoothing,
                                long long bg_index, int reduction, int accumulate_loss, float* workspace, size_t ws_floats,
                                void* stream) {
    C2S_REQUIRE(logits && target && loss && workspace, "smooth_ce: null pointer");
    C2S_REQUIRE(B > 0 && H > 0 && W > 0 && K >= 1 && K <= MAXK, "smooth_ce: 1 <= K <= 32 classes");
    C2S_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, "smooth_ce: label_smoothing outside [0, 1]");
    C2S_REQUIRE(reduction >= 0 && reduction <= 2 && (reduction != 2 || pixel_loss != nullptr), "smooth_ce: reduction 0 mean / 1 sum / 2 none (needs pixel_loss)");
    C2S_REQUIRE(ws_floats >= c2s_smooth_ce_workspace_floats(), "smooth_ce: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid_for((long)B * H * W, LOSS_BLOCKS);
    float* tot = workspace + 2 * LOSS_BLOCKS;
    const double npix = reduction == 0 ? (double)B * H * W : 1.0;
    hipLaunchKernelGGL(smooth_ce_kernel, dim3(blocks), dim3(256), 0, st, logits, (const int64_t*)target, class_w, bg_distrib,
                       workspace, glogits, pixel_loss, B, K, H, W, label_smoothing, bg_index, (float)(1.0 / npix));
    C2S_CHECK_LAUNCH("smooth_ce");
    hipLaunchKernelGGL(smooth_ce_finalize_kernel, dim3(1), dim3(64), 0, st, workspace, tot, loss, blocks, npix, accumulate_loss);
    C2S_CHECK_LAUNCH("smooth_ce_finalize");
    return C2S_OK;
}

extern "C" int c2s_smooth_ce(const float* logits, const long long* target, const float* class_w, const float* bg_distrib,
                             float* loss, float* glogits, int B, int K, int H, int W, float label_smoothing,
                             long long bg_index, int accumulate_loss, float* workspace, size_t ws_floats, void* stream) {
    return c2s_smooth_ce_ex(logits, target, class_w, bg_distrib, loss, glogits, nullptr, B, K, H, W, label_smoothing, bg_index, 0,
                            accumulate_loss, workspace, ws_floats, stream);
}

extern "C" size_t c2s_recall_ce_workspace_floats(int B, int HW) {
    return (B > 0 && HW > 0) ? recall_ws_floats((long)B * HW) : recall_ws_floats(0);
}

extern "C" int c2s_recall_ce(const float* logits, const long long* target, float* loss, float* glogits, float* weights_out,
                             long long* counts_out, int B, int K, int HW, long long ignore_index, int accumulate_loss,
                             float* workspace, size_t ws_floats, void* stream) {
    C2S_REQUIRE(K >= 1 && K <= MAXK, "recall_ce: 1 <= K <= 32 classes (got %d)", K);
    C2S_REQUIRE(logits && target && loss && workspace, "recall_ce: null pointer");
    C2S_REQUIRE(B > 0 && HW > 0, "recall_ce: bad args");
    C2S_REQUIRE(ws_floats >= c2s_recall_ce_workspace_floats(B, HW), "recall_ce: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)B * HW;
    const int blocks = grid_for(n, LOSS_BLOCKS);
    float* nll = workspace;
    float* part = workspace + n;
    float* cnt_f = part + LOSS_BLOCKS;
    if (((uintptr_t)cnt_f & 7) != 0) ++cnt_f;                 // the slack float: 64-bit atomics need 8-byte alignment
    unsigned long long* cnt = (unsigned long long*)cnt_f;
    float* w = part + LOSS_BLOCKS + (2 * NCOUNT + 1);
    float* tot = w + MAXK;                                    // (sum of w_t nll, targets outside [0,K) other than ignore_index)
    hipLaunchKernelGGL(recall_zero_kernel, dim3(1), dim3(128), 0, st, cnt);
    C2S_CHECK_LAUNCH("recall_zero");
    hipLaunchKernelGGL(recall_count_kernel, dim3(blocks), dim3(256), 0, st, logits, (const int64_t*)target, nll, cnt, B, K, HW,
                       ignore_index);
    C2S_CHECK_LAUNCH("recall_count");
    hipLaunchKernelGGL(recall_weights_kernel, dim3(1), dim3(64), 0, st, cnt, w, tot, weights_out, counts_out, K);
    C2S_CHECK_LAUNCH("recall_weights");
    hipLaunchKernelGGL(recall_loss_kernel, dim3(blocks), dim3(256), 0, st, nll, (const int64_t*)target, w, part, n, K,
                       ignore_index);
    C2S_CHECK_LAUNCH("recall_loss");
    hipLaunchKernelGGL(recall_finalize_kernel, dim3(1), dim3(64), 0, st, part, tot, loss, blocks, (double)n, accumulate_loss);
    C2S_CHECK_LAUNCH("recall_finalize");
    if (glogits != nullptr) {
        hipLaunchKernelGGL(recall_bwd_kernel, dim3(blocks), dim3(256), 0, st, logits, (const int64_t*)target, w, glogits, B, K, HW,
                           ignore_index, (float)(1.0 / (double)n));
        C2S_CHECK_LAUNCH("recall_bwd");
    }
    return C2S_OK;
}
