// RecallCrossEntropy (reference src/learning/recall_loss.py:8-50; arXiv 2106.14917): cross entropy weighted per class by the
// batch's false-negative share,
//   pred = argmax_k z_k (first maximum, NaN counts as the maximum: metrics_update_kernel's rule == torch.argmax)
//   gt_c = #{valid pixels with t = c},  fn_c = #{valid pixels with t = c and pred != c}
//   w_c  = max(fn_c, 1) / max(gt_c, 1)            (the reference's counters start from torch.ones, :28,37)
//   loss = (1 / N) sum_valid w_t (lse(z) - z_t),   N = B*H*W: ALL pixels (the reference's .mean() of a reduction='none' tensor)
//   dL/dz_k = (w_t / N) (p_k - [k = t]) on valid pixels, 0 elsewhere: the weights come from an argmax and are constants.
// A pixel is valid when its target lies in [0, K) and is not ignore_index; other targets outside [0, K) are counted ("bad").
//
// The weights need a reduction over the whole batch before any pixel's term is known, so the pass is split:
//   recall_zero_kernel     zeroes the counters (a kernel, not a memset: a replayed hipGraph zeroes them again)
//   recall_count_kernel    the first read of the logits: argmax, nll per pixel -> workspace, LDS histograms gt / fn / bad,
//                          one 64-bit integer atomic per non-zero bin (order independent, bit-exact)
//   recall_weights_kernel  w_c, published with the counts
//   recall_loss_kernel     float block partials of w_t nll in ce_fwd_kernel's fixed order; recall_finalize_kernel in double
//   recall_bwd_kernel      the second and last read of the logits
// No float atomics: loss and gradient are bitwise reproducible from run to run.  Everything is stream-ordered.
#include "common.h"

namespace {

constexpr int MAXK = 32;                  // metrics.hip's MAXK
constexpr int RECALL_BLOCKS = 512;        // grid cap of the three per-pixel kernels
constexpr int NCOUNT = 2 * MAXK + 1;      // gt[MAXK], fn[MAXK], bad

// Workspace (floats), n = B*HW:
//   [0, n) nll | [n, n + RECALL_BLOCKS) block partials | NCOUNT 64-bit counters in 2*NCOUNT + 1 floats (one float of slack:
//   the counters start at the first 8-byte boundary) | w[MAXK] | (sum of w_t nll, bad-label count)
inline size_t ws_floats_for(long n) { return (size_t)n + RECALL_BLOCKS + (2 * NCOUNT + 1) + MAXK + 2; }

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
        if (t == ignore_index || t < 0 || t >= K) {
            if (t != ignore_index) atomicAdd(&h[2 * MAXK], 1u);
            nll[e] = 0.f;
            continue;
        }
        const int pix = (int)(e % HW), b = (int)(e / HW);
        float v[MAXK];
        load_pixel(logits + (size_t)b * K * HW + pix, K, HW, v);
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
    __shared__ float red[4];
    __shared__ float ws[MAXK];
    if (threadIdx.x < K) ws[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    float num = 0.f;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long long t = target[e];
        if (t == ignore_index || t < 0 || t >= K) continue;
        num += ws[(int)t] * nll[e];
    }
    num = wave_sum(num);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = num;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void recall_finalize_kernel(const float* __restrict__ part, float* __restrict__ tot, float* __restrict__ loss,
                                       int blocks, double npix, int accumulate) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double num = 0;
    for (int i = 0; i < blocks; ++i) num += part[i];
    tot[0] = (float)num;
    const float l = (float)(num / npix);
    *loss = accumulate ? *loss + l : l;
}

__global__ __launch_bounds__(256) void recall_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                         const float* __restrict__ w, float* __restrict__ glogits, int B, int K,
                                                         int HW, long long ignore_index, float inv_n) {
    __shared__ float ws[MAXK];
    if (threadIdx.x < K) ws[threadIdx.x] = w[threadIdx.x];
    __syncthreads();
    const long total = (long)B * HW;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int pix = (int)(e % HW), b = (int)(e / HW);
        float* gp = glogits + (size_t)b * K * HW + pix;
        const long long t = target[e];
        if (t == ignore_index || t < 0 || t >= K) {
            for (int k = 0; k < K; ++k) gp[(size_t)k * HW] = 0.f;
            continue;
        }
        float v[MAXK];
        load_pixel(logits + (size_t)b * K * HW + pix, K, HW, v);
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

inline int grid_for(long n, int cap) {
    long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" size_t c2s_recall_ce_workspace_floats(int B, int HW) {
    return (B > 0 && HW > 0) ? ws_floats_for((long)B * HW) : ws_floats_for(0);
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
    const int blocks = grid_for(n, RECALL_BLOCKS);
    float* nll = workspace;
    float* part = workspace + n;
    float* cnt_f = part + RECALL_BLOCKS;
    if (((uintptr_t)cnt_f & 7) != 0) ++cnt_f;                 // the slack float: 64-bit atomics need 8-byte alignment
    unsigned long long* cnt = (unsigned long long*)cnt_f;
    float* w = part + RECALL_BLOCKS + (2 * NCOUNT + 1);
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
