// Parcel homogenisation of predictions (the raster restatement of src/helpers/postprocess.py:377-604).
//
// Reference call sites (paths under the reference root):
//   src/helpers/postprocess.py:540-551  top-2 of the class probabilities; super = not (boundary | strong second boundary | class 0)
//   src/helpers/postprocess.py:532-536,554-560  scipy.ndimage.label with the plus element; components under 13 pixels removed
//   src/helpers/postprocess.py:449-456,580  per parcel: the class of the largest area; background only above a 0.75 share
//   src/helpers/postprocess.py:238-281,491-507  type_='soft': per parcel the mean of the class probabilities of its pixels;
//                                          the class of the largest mean, the runner-up kept; background only above 0.7
//   src/learning/utils.py:341-361,383   iterate(): the homogenised prediction feeds the IoU meter
//
// A parcel is a set of pixels with one integer id and an area is a pixel count, so everything after the seeds rule is
// integer work: bit-exact and independent of scheduling (the soft vote sums its probabilities in 64-bit fixed point for the
// same reason).  All rasters are [B,H,W]; images are independent.  Every pass is one thread per pixel over a few bytes per
// pixel (latency- and atomic-bound, not bandwidth-bound; the soft vote's sum reads all K scores of a parcel pixel); entry
// points only enqueue on the stream: no allocation, no read-back, no synchronisation.
#include <float.h>
#include <limits.h>
#include "common.h"
#include "parcels_uf.h"

namespace {

constexpr int PC_SCAN = 256;    // pixels one workgroup of the numbering scan covers (one per lane)
constexpr int PC_BLOCKS = 4096; // grid cap of the grid-stride kernels
constexpr long PC_MAX_PIXELS = INT_MAX - (long)PC_BLOCKS * 256;       // a grid-stride step past the last pixel still fits an int

// base[key] += number of active lanes of the wave that hold `key`: one atomic per distinct key and wave.  Called by whole
// waves (the callers' loops have wave-uniform trip counts).
__device__ __forceinline__ void wave_count_add(int* __restrict__ base, int key, bool on) {
    unsigned long long todo = __ballot(on);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(on && key == k0);
        if (lane == leader) atomicAdd(base + k0, (int)__popcll(same));
        todo &= ~same;
    }
}

// inclusive prefix sum of v over the 256 lanes of the workgroup; total = the sum.  sw: 4 ints of LDS.
__device__ __forceinline__ int block_scan_incl(int v, int* sw, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                            // the previous use of sw is over
    if (lane == 63) sw[w] = x;
    __syncthreads();
    int off = 0;
    for (int j = 0; j < w; ++j) off += sw[j];
    total = sw[0] + sw[1] + sw[2] + sw[3];
    return x + off;
}

// ---------------------------------------------------------------- (a) seeds (postprocess.py:540-551)
// top-1 / top-2 as metrics_update_kernel finds them: first maximum, lowest index on ties.  With from_logits the softmax
// runs here (max-subtracted, fp32, as softmax_stitch_kernel).
__global__ __launch_bounds__(256) void parcel_seeds_kernel(const float* __restrict__ scores, const float* __restrict__ bscores,
                                                           unsigned char* __restrict__ mask, int64_t* __restrict__ t1_out,
                                                           int B, int K, int HW, int from_logits, int boundary_code,
                                                           float thr) {
    const long total = (long)B * HW;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int pix = (int)(e % HW), b = (int)(e / HW);
        const float* sp = scores + (size_t)b * K * HW + pix;
        float v1 = sp[0], v2 = -INFINITY;
        int i1 = 0, i2 = -1;
        for (int k = 1; k < K; ++k) {
            const float v = sp[(size_t)k * HW];
            if (v > v1 || (v != v && v1 == v1)) {
                v2 = v1; i2 = i1; v1 = v; i1 = k;
            } else if (i2 < 0 || v > v2 || (v != v && v2 == v2)) {
                v2 = v; i2 = k;
            }
        }
        float p2 = v2;
        if (from_logits) {
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += expf(sp[(size_t)k * HW] - v1);
            p2 = expf(v2 - v1) / s;
        }
        bool boundary;
        if (bscores) {                                      // the separate 2-class head
            const float* bp = bscores + (size_t)b * 2 * HW + pix;
            float p0 = bp[0], p1 = bp[HW];
            if (from_logits) {
                const float m = fmaxf(p0, p1);
                const float e0 = expf(p0 - m), e1 = expf(p1 - m);
                p0 = e0 / (e0 + e1);
                p1 = e1 / (e0 + e1);
            }
            boundary = p1 >= p0 || p1 > thr;
        } else {
            boundary = i1 == boundary_code || (i2 == boundary_code && p2 > thr);
        }
        mask[e] = (boundary || i1 == 0) ? 0 : 1;
        if (t1_out) t1_out[e] = i1;
    }
}

// ---------------------------------------------------------------- (b) connected components, 4-connectivity
__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ parent, int* __restrict__ size, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) { parent[i] = i; size[i] = 0; }
}

__global__ __launch_bounds__(256) void cc_unite_kernel(int* __restrict__ parent, const unsigned char* __restrict__ mask, int n,
                                                       int H, int W, int* __restrict__ error) {
    const int cap = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        if (mask[i] && !puf_unite_pixel(parent, mask, i, H, W, cap)) atomicOr(error, 1);
}

// parent[i] = the root; size[root] = pixels of the component
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* __restrict__ parent, int* __restrict__ size,
                                                         const unsigned char* __restrict__ mask, int n, int H, int W,
                                                         int* __restrict__ error) {
    const int cap = H * W;
    for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {      // wave-uniform: wave_count_add
        const int i = base + threadIdx.x;
        const bool on = i < n && mask[i];
        int r = 0;
        if (on) {
            r = puf_find(parent, i, cap);
            if (r < 0) { atomicOr(error, 1); r = i; }
            parent[i] = r;
        }
        wave_count_add(size, r, on);
    }
}

__device__ __forceinline__ bool cc_survivor(const int* __restrict__ parent, const int* __restrict__ size,
                                            const unsigned char* __restrict__ mask, int i, int min_size) {
    return mask[i] && parent[i] == i && size[i] >= min_size;
}

// grid (blocks per image, B): sums[b][block] = surviving roots among the block's PC_SCAN pixels
__global__ __launch_bounds__(PC_SCAN) void cc_count_kernel(const int* __restrict__ parent, const int* __restrict__ size,
                                                           const unsigned char* __restrict__ mask, int HW, int min_size,
                                                           int* __restrict__ sums) {
    __shared__ int sw[4];
    const int p = blockIdx.x * PC_SCAN + threadIdx.x;
    const int i = blockIdx.y * HW + p;
    int total;
    block_scan_incl(p < HW && cc_survivor(parent, size, mask, i, min_size) ? 1 : 0, sw, total);
    if (threadIdx.x == 0) sums[blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// one workgroup per image: sums[b][*] -> their exclusive prefix sums, count[b] = the image's components
__global__ __launch_bounds__(256) void cc_scan_sums_kernel(int* __restrict__ sums, int nblk, int* __restrict__ count) {
    __shared__ int sw[4];
    int* s = sums + (size_t)blockIdx.x * nblk;
    int carry = 0;
    for (int base = 0; base < nblk; base += 256) {
        const int j = base + threadIdx.x;
        const int v = j < nblk ? s[j] : 0;
        int total;
        const int incl = block_scan_incl(v, sw, total);
        if (j < nblk) s[j] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

// size[root] = the dense id of a surviving root (1..n in raster order of the roots = of the components' first pixels), 0
// for a removed one
__global__ __launch_bounds__(PC_SCAN) void cc_number_kernel(const int* __restrict__ parent, int* __restrict__ size,
                                                            const unsigned char* __restrict__ mask, int HW, int min_size,
                                                            const int* __restrict__ sums) {
    __shared__ int sw[4];
    const int p = blockIdx.x * PC_SCAN + threadIdx.x;
    const int i = blockIdx.y * HW + p;
    const bool in = p < HW;
    const bool root = in && mask[i] && parent[i] == i;
    const bool on = root && size[i] >= min_size;
    int total;
    const int incl = block_scan_incl(on ? 1 : 0, sw, total);
    if (root) size[i] = on ? sums[blockIdx.y * gridDim.x + blockIdx.x] + incl : 0;
}

__global__ __launch_bounds__(256) void cc_write_kernel(const int* __restrict__ parent, const int* __restrict__ ids,
                                                       const unsigned char* __restrict__ mask, int* __restrict__ labels, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) labels[i] = mask[i] ? ids[parent[i]] : 0;
}

// ---------------------------------------------------------------- (c) the vote (postprocess.py:449-456,580)
__global__ __launch_bounds__(256) void vote_zero_kernel(int* __restrict__ hist, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) hist[i] = 0;
}

// hist[b][label-1][pred] += 1; error[0] += labels outside [0, cap], error[1] += classes outside [0, K)
__global__ __launch_bounds__(256) void vote_hist_kernel(const int64_t* __restrict__ pred, const int* __restrict__ labels,
                                                        int* __restrict__ hist, int n, int HW, int K, int cap,
                                                        int* __restrict__ error) {
    for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {      // wave-uniform: wave_count_add
        const int i = base + threadIdx.x;
        bool on = false, bad_label = false, bad_class = false;
        int key = 0;
        if (i < n) {
            const int l = labels[i];
            const long long c = pred[i];
            bad_label = l < 0 || l > cap;
            bad_class = c < 0 || c >= K;
            on = l > 0 && !bad_label && !bad_class;
            if (on) key = ((i / HW) * cap + (l - 1)) * K + (int)c;
        }
        wave_count_add(hist, key, on);
        wave_count_add(error, 0, bad_label);
        wave_count_add(error, 1, bad_class);
    }
}

// one thread per parcel: the candidate class of the largest count, lower class on ties, 0 without a candidate
__global__ __launch_bounds__(256) void vote_winner_kernel(const int* __restrict__ hist, int* __restrict__ parcel_class,
                                                          int nparcels, int K, float bg_share) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < nparcels; p += gridDim.x * 256) {
        const int* h = hist + (size_t)p * K;
        long total = 0;
        for (int k = 0; k < K; ++k) total += h[k];
        int best = 0, win = 0;
        if (bg_share >= 0.f && h[0] > 0 && (double)h[0] > (double)bg_share * (double)total) best = h[0];
        for (int k = 1; k < K; ++k)
            if (h[k] > best) { best = h[k]; win = k; }
        parcel_class[p] = win;
    }
}

__global__ __launch_bounds__(256) void vote_write_kernel(const int64_t* __restrict__ pred, const int* __restrict__ labels,
                                                         const int* __restrict__ parcel_class, int64_t* __restrict__ out, int n,
                                                         int HW, int K, int cap, int outside) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int l = labels[i];
        const long long c = pred[i];
        if (l < 0 || l > cap || c < 0 || c >= K) continue;             // counted by vote_hist_kernel: nothing is written
        out[i] = l > 0 ? (long long)parcel_class[(i / HW) * cap + (l - 1)] : (outside ? c : 0);
    }
}

// ---------------------------------------------------------------- (d) the soft vote (postprocess.py:238-281,491-507)
// Every live pixel (label in [1, cap], all K scores finite) adds q(p_k) = rint(clamp(p_k, 0, 1) * 2^32) to the 64-bit sum
// S[b][label-1][k] of every class and 1 to n[b][label-1]: integer sums, so the result does not depend on arrival order.
// q(1.0) = 2^32 does not fit 32 bits; n < 2^31 keeps S below 2^63.
typedef unsigned long long u64;

constexpr int PS_ITER = 4;      // consecutive 256-pixel rows one workgroup of the summing kernel covers
constexpr int PS_GROUPS = 4;    // distinct ids per wave that are summed across the wave; further ids add lane by lane

// one butterfly step: lanes OFF apart exchange halves of the HALF * 2 classes they still keep (compile-time indices only)
template <int HALF, int OFF, int KP>
__device__ __forceinline__ void soft_fold(u64 (&c)[KP], int lane) {
    if constexpr (HALF >= 1) {
        const bool up = (lane & OFF) != 0;                  // upper lanes keep the upper half of the classes
#pragma unroll
        for (int j = 0; j < HALF; ++j) {
            const u64 keep = up ? c[j + HALF] : c[j];
            const u64 send = up ? c[j] : c[j + HALF];
            c[j] = keep + __shfl_xor(send, OFF, 64);
        }
        soft_fold<HALF / 2, OFF / 2, KP>(c, lane);
    } else if constexpr (OFF >= 1) {
        c[0] += __shfl_xor(c[0], OFF, 64);
        soft_fold<0, OFF / 2, KP>(c, lane);
    }
}

// Sum over the lanes with `mine` of q[k], for every class at once.  A butterfly that halves the classes a lane keeps at
// every step: KP - 1 exchanges for the first log2(KP) steps, one each for the rest.  Returns, in every lane, the sum of
// class (lane >> (6 - log2 KP)).  Called by whole waves.
template <int KP>
__device__ __forceinline__ u64 wave_class_sums(const u64 (&q)[KP], bool mine) {
    const int lane = threadIdx.x & 63;
    u64 c[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) c[k] = mine ? q[k] : 0ull;
    soft_fold<KP / 2, 32, KP>(c, lane);
    return c[0];
}

// the sums a wave holds for parcel `key` (class lane >> SH in the lanes whose low SH bits are 0) and its pixel count
template <int KP>
__device__ __forceinline__ void soft_flush(u64* __restrict__ S, int* __restrict__ cnt, int key, u64 sum, int n, int K) {
    constexpr int SH = KP == 32 ? 1 : KP == 16 ? 2 : KP == 8 ? 3 : 4;          // 6 - log2 KP
    const int lane = threadIdx.x & 63, k = lane >> SH;
    if (key < 0) return;
    if ((lane & ((1 << SH) - 1)) == 0 && k < K && sum) atomicAdd(S + (size_t)key * K + k, sum);
    if (lane == 0 && n) atomicAdd(cnt + key, n);
}

// One thread per pixel, a workgroup over PS_ITER * 256 consecutive pixels.  A thread reads each class of its pixel once
// (coalesced across lanes in the [K,HW] layout); with from_logits the softmax runs here as in parcel_seeds_kernel (fp32,
// max-subtracted).  Equal ids of a wave are summed on chip (wave_class_sums), and while a wave keeps meeting the same id
// from one 256-pixel row to the next the sums and the pixel count stay in registers; what the four waves still hold at the
// end is merged through LDS where they hold the same id.  So a parcel wider than the workgroup's span costs one 64-bit
// atomic per class and workgroup, a small one one per class and wave that meets it.
// error[0] += labels outside [0, cap], error[2] += live pixels with a non-finite score.
template <int KP>
__global__ __launch_bounds__(256) void soft_sum_kernel(const float* __restrict__ scores, const int* __restrict__ labels,
                                                       u64* __restrict__ S, int* __restrict__ cnt, long total, int HW, int K,
                                                       int cap, int from_logits, int* __restrict__ error) {
    constexpr int SH = KP == 32 ? 1 : KP == 16 ? 2 : KP == 8 ? 3 : 4;
    __shared__ u64 wsum[4][KP];
    __shared__ int wkey[4], wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int pend_key = -1, pend_n = 0;                          // wave-uniform: the id whose sums `pend` holds, and its pixels
    u64 pend = 0;
    const long first = blockIdx.x * (256L * PS_ITER);
    for (int it = 0; it < PS_ITER; ++it) {
        const long base = first + it * 256L;
        if (base >= total) break;                           // uniform over the workgroup
        const long e = base + threadIdx.x;
        bool on = false, bad_label = false, bad_score = false;
        int key = 0;
        u64 q[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) q[k] = 0;
        if (e < total) {
            const int b = (int)(e / HW), pix = (int)(e - (long)b * HW);
            const int l = labels[e];
            bad_label = l < 0 || l > cap;
            if (l > 0 && !bad_label) {
                const float* sp = scores + (size_t)b * K * HW + pix;
                float v[KP];
                bool finite = true;
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    v[k] = k < K ? sp[(size_t)k * HW] : 0.f;
                    finite = finite && fabsf(v[k]) <= FLT_MAX;          // false for NaN and both infinities
                }
                on = finite;
                bad_score = !finite;
                key = b * cap + (l - 1);
                if (on) {
                    if (from_logits) {
                        float m = v[0], s = 0.f;
#pragma unroll
                        for (int k = 1; k < KP; ++k)
                            if (k < K && v[k] > m) m = v[k];
#pragma unroll
                        for (int k = 0; k < KP; ++k)
                            if (k < K) { v[k] = expf(v[k] - m); s += v[k]; }
#pragma unroll
                        for (int k = 0; k < KP; ++k) v[k] = v[k] / s;
                    }
#pragma unroll
                    for (int k = 0; k < KP; ++k)
                        if (k < K) q[k] = (u64)rintf(fminf(fmaxf(v[k], 0.f), 1.f) * 4294967296.f);
                }
            }
        }
        wave_count_add(error, 0, bad_label);
        wave_count_add(error, 2, bad_score);
        u64 todo = __ballot(on);
        for (int g = 0; g < PS_GROUPS && todo; ++g) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k0 = __shfl(key, leader, 64);
            const bool mine = on && key == k0;
            const u64 c = wave_class_sums<KP>(q, mine);
            const u64 same = __ballot(mine);
            if (k0 != pend_key) {
                soft_flush<KP>(S, cnt, pend_key, pend, pend_n, K);
                pend_key = k0;
                pend = 0;
                pend_n = 0;
            }
            pend += c;
            pend_n += (int)__popcll(same);
            todo &= ~same;
        }
        const bool left = (todo >> lane) & 1;               // more than PS_GROUPS ids in this wave: lanes rarely share one
        if (left) {
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K && q[k]) atomicAdd(S + (size_t)key * K + k, q[k]);
        }
        wave_count_add(cnt, key, left);
    }
    // merge what the four waves hold: the first wave with an id adds for all that hold it
    if ((lane & ((1 << SH) - 1)) == 0) wsum[wave][lane >> SH] = pend;
    if (lane == 0) { wkey[wave] = pend_key; wcnt[wave] = pend_n; }
    __syncthreads();
    bool mine_to_add = pend_key >= 0;
    for (int w = 0; w < wave; ++w) mine_to_add = mine_to_add && wkey[w] != pend_key;
    if (mine_to_add) {
        for (int w = wave + 1; w < 4; ++w)
            if (wkey[w] == pend_key) { pend += wsum[w][lane >> SH]; pend_n += wcnt[w]; }
        soft_flush<KP>(S, cnt, pend_key, pend, pend_n, K);
    }
}

__global__ __launch_bounds__(256) void soft_zero_kernel(unsigned* __restrict__ p, size_t n) {
    for (size_t i = blockIdx.x * 256ul + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

// one thread per parcel: classes ordered by (sum descending, class ascending) -> t1, t2; the label is t1 unless t1 is the
// background and its mean is not strictly above bg_mean (soften's `> 0.7`), then t2; top2 = t2 either way
__global__ __launch_bounds__(256) void soft_winner_kernel(const u64* __restrict__ S, const int* __restrict__ cnt,
                                                          int* __restrict__ parcel_label, int* __restrict__ parcel_top2,
                                                          float* __restrict__ parcel_mean, int* __restrict__ parcel_pixels,
                                                          int nparcels, int K, float bg_mean) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < nparcels; p += gridDim.x * 256) {
        const u64* s = S + (size_t)p * K;
        float* mean = parcel_mean + (size_t)p * K;
        const int n = cnt[p];
        parcel_pixels[p] = n;
        if (n == 0) {
            parcel_label[p] = 0;
            parcel_top2[p] = 0;
            for (int k = 0; k < K; ++k) mean[k] = 0.f;
            continue;
        }
        int t1 = 0, t2 = -1;
        u64 s1 = s[0], s2 = 0;
        for (int k = 1; k < K; ++k) {
            const u64 v = s[k];
            if (v > s1) {
                t2 = t1; s2 = s1; t1 = k; s1 = v;
            } else if (t2 < 0 || v > s2) {
                t2 = k; s2 = v;
            }
        }
        const double den = (double)n * 4294967296.0;
        for (int k = 0; k < K; ++k) mean[k] = (float)((double)s[k] / den);
        const bool bg = (double)s[0] > (double)bg_mean * (double)n * 4294967296.0;
        parcel_label[p] = (t1 == 0 && !bg) ? t2 : t1;
        parcel_top2[p] = t2;
    }
}

__global__ __launch_bounds__(256) void soft_write_kernel(const float* __restrict__ scores, const int* __restrict__ labels,
                                                         const int* __restrict__ parcel_label, int64_t* __restrict__ out, int n,
                                                         int HW, int K, int cap, int outside) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int l = labels[i];
        if (l < 0 || l > cap) continue;                     // counted by soft_sum_kernel: nothing is written
        const int b = i / HW;
        long long c = 0;
        if (l > 0) {
            c = parcel_label[b * cap + (l - 1)];
        } else if (outside) {                               // the pixel's own top-1, as parcel_seeds_kernel finds it
            const float* sp = scores + (size_t)b * K * HW + (i - b * HW);
            float v1 = sp[0];
            for (int k = 1; k < K; ++k) {
                const float v = sp[(size_t)k * HW];
                if (v > v1 || (v != v && v1 == v1)) { v1 = v; c = k; }
            }
        }
        out[i] = c;
    }
}

inline long cc_pixels(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const long n = (long)B * H * W;
    return n <= PC_MAX_PIXELS && B <= 65535 ? n : 0;        // int indices; grid.y = B
}

}  // namespace

extern "C" int c2s_parcel_seeds(const float* scores, const float* boundary_scores, unsigned char* mask, long long* t1, int B,
                                int K, int H, int W, int from_logits, int boundary_code, float second_threshold,
                                void* stream) {
    C2S_REQUIRE(scores && mask, "parcel_seeds: null pointer");
    C2S_REQUIRE(B > 0 && H > 0 && W > 0 && (long)H * W <= INT_MAX, "parcel_seeds: bad shape");
    C2S_REQUIRE(K >= 2 && K <= C2S_MAX_CLASSES, "parcel_seeds: 2 <= K <= 32 classes");
    C2S_REQUIRE(from_logits == 0 || from_logits == 1, "parcel_seeds: from_logits is 0 or 1");
    C2S_REQUIRE(!(second_threshold != second_threshold), "parcel_seeds: second_threshold is NaN");
    hipLaunchKernelGGL(parcel_seeds_kernel, dim3(grid_for((long)B * H * W, PC_BLOCKS)), dim3(256), 0, (hipStream_t)stream, scores,
                       boundary_scores, mask, (int64_t*)t1, B, K, H * W, from_logits, boundary_code, second_threshold);
    C2S_CHECK_LAUNCH("parcel_seeds");
    return C2S_OK;
}

// parent int[n] | size / id int[n] | block sums int[B * blocks per image]
extern "C" size_t c2s_label_components_workspace_bytes(int B, int H, int W) {
    const long n = cc_pixels(B, H, W);
    if (n == 0) return 0;
    const long nblk = ((long)H * W + PC_SCAN - 1) / PC_SCAN;
    return (size_t)(2 * n + B * nblk) * sizeof(int);
}

extern "C" int c2s_label_components(const unsigned char* mask, int* labels, int* count, int B, int H, int W, int min_size,
                                    void* workspace, size_t ws_bytes, int* error, void* stream) {
    C2S_REQUIRE(mask && labels && count && workspace && error, "label_components: null pointer");
    const long nl = cc_pixels(B, H, W);
    C2S_REQUIRE(nl > 0, "label_components: bad shape (B * H * W <= %ld, B <= 65535)", PC_MAX_PIXELS);
    C2S_REQUIRE(min_size >= 1, "label_components: min_size %d < 1", min_size);
    C2S_REQUIRE((uintptr_t)workspace % 16 == 0, "label_components: workspace not 16-byte aligned");
    const size_t need = c2s_label_components_workspace_bytes(B, H, W);
    C2S_REQUIRE(ws_bytes >= need, "label_components: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int n = (int)nl, HW = H * W, nblk = (HW + PC_SCAN - 1) / PC_SCAN;
    int* parent = (int*)workspace;
    int* size = parent + n;
    int* sums = size + n;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(grid_for(n, PC_BLOCKS)), t(256), gs(nblk, B);
    hipLaunchKernelGGL(cc_init_kernel, g, t, 0, st, parent, size, n);
    C2S_CHECK_LAUNCH("cc_init");
    hipLaunchKernelGGL(cc_unite_kernel, g, t, 0, st, parent, mask, n, H, W, error);
    C2S_CHECK_LAUNCH("cc_unite");
    hipLaunchKernelGGL(cc_flatten_kernel, g, t, 0, st, parent, size, mask, n, H, W, error);
    C2S_CHECK_LAUNCH("cc_flatten");
    hipLaunchKernelGGL(cc_count_kernel, gs, dim3(PC_SCAN), 0, st, parent, size, mask, HW, min_size, sums);
    C2S_CHECK_LAUNCH("cc_count");
    hipLaunchKernelGGL(cc_scan_sums_kernel, dim3(B), t, 0, st, sums, nblk, count);
    C2S_CHECK_LAUNCH("cc_scan_sums");
    hipLaunchKernelGGL(cc_number_kernel, gs, dim3(PC_SCAN), 0, st, parent, size, mask, HW, min_size, sums);
    C2S_CHECK_LAUNCH("cc_number");
    hipLaunchKernelGGL(cc_write_kernel, g, t, 0, st, parent, size, mask, labels, n);
    C2S_CHECK_LAUNCH("cc_write");
    return C2S_OK;
}

// the histogram int[B][cap][K]
extern "C" size_t c2s_parcel_vote_workspace_bytes(int B, int cap, int K) {
    if (B <= 0 || cap <= 0 || K <= 0) return 0;
    const long n = (long)B * cap * K;
    return n <= INT_MAX ? (size_t)n * sizeof(int) : 0;
}

extern "C" int c2s_parcel_vote(const long long* pred, const int* labels, long long* out, int* parcel_class, int B, int H, int W,
                               int K, int cap, float bg_share, int outside, void* workspace, size_t ws_bytes, int* error,
                               void* stream) {
    C2S_REQUIRE(pred && labels && out && parcel_class && workspace && error, "parcel_vote: null pointer");
    C2S_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W <= PC_MAX_PIXELS, "parcel_vote: bad shape (B * H * W <= %ld)", PC_MAX_PIXELS);
    C2S_REQUIRE(K >= 2 && K <= C2S_MAX_CLASSES, "parcel_vote: 2 <= K <= 32 classes");
    C2S_REQUIRE(cap >= 1, "parcel_vote: cap %d < 1", cap);
    C2S_REQUIRE(outside == 0 || outside == 1, "parcel_vote: outside is 0 (zero) or 1 (keep)");
    C2S_REQUIRE(!(bg_share != bg_share), "parcel_vote: bg_share is NaN");
    const size_t need = c2s_parcel_vote_workspace_bytes(B, cap, K);
    C2S_REQUIRE(need > 0, "parcel_vote: B * cap * K = %ld entries are more than int indices reach", (long)B * cap * K);
    C2S_REQUIRE((uintptr_t)workspace % 16 == 0, "parcel_vote: workspace not 16-byte aligned");
    C2S_REQUIRE(ws_bytes >= need, "parcel_vote: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int n = B * H * W, HW = H * W, nh = B * cap * K;
    int* hist = (int*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(grid_for(n, PC_BLOCKS)), t(256);
    hipLaunchKernelGGL(vote_zero_kernel, dim3(grid_for(nh, PC_BLOCKS)), t, 0, st, hist, nh);
    C2S_CHECK_LAUNCH("vote_zero");
    hipLaunchKernelGGL(vote_hist_kernel, g, t, 0, st, (const int64_t*)pred, labels, hist, n, HW, K, cap, error);
    C2S_CHECK_LAUNCH("vote_hist");
    hipLaunchKernelGGL(vote_winner_kernel, dim3(grid_for((long)B * cap, PC_BLOCKS)), t, 0, st, hist, parcel_class, B * cap, K, bg_share);
    C2S_CHECK_LAUNCH("vote_winner");
    hipLaunchKernelGGL(vote_write_kernel, g, t, 0, st, (const int64_t*)pred, labels, parcel_class, (int64_t*)out, n, HW, K, cap,
                       outside);
    C2S_CHECK_LAUNCH("vote_write");
    return C2S_OK;
}

// the sums u64[B][cap][K] | the pixel counts int[B][cap], rounded up to 16 bytes
extern "C" size_t c2s_parcel_soft_vote_workspace_bytes(int B, int cap, int K) {
    if (B <= 0 || cap <= 0 || K <= 0) return 0;
    const long n = (long)B * cap * K;
    if (n > INT_MAX) return 0;
    const size_t bytes = (size_t)n * sizeof(u64) + (size_t)B * cap * sizeof(int);
    return (bytes + 15) / 16 * 16;
}

extern "C" int c2s_parcel_soft_vote(const float* scores, const int* labels, long long* out, int* parcel_label, int* parcel_top2,
                                    float* parcel_mean, int* parcel_pixels, int B, int K, int H, int W, int cap, int from_logits,
                                    float bg_mean, int outside, void* workspace, size_t ws_bytes, int* error, void* stream) {
    C2S_REQUIRE(scores && labels && out && parcel_label && parcel_top2 && parcel_mean && parcel_pixels && workspace && error,
                "parcel_soft_vote: null pointer");
    C2S_REQUIRE(B > 0 && H > 0 && W > 0 && (long)B * H * W <= PC_MAX_PIXELS, "parcel_soft_vote: bad shape (B * H * W <= %ld)", PC_MAX_PIXELS);
    C2S_REQUIRE(K >= 2 && K <= C2S_MAX_CLASSES, "parcel_soft_vote: 2 <= K <= 32 classes");
    C2S_REQUIRE(cap >= 1, "parcel_soft_vote: cap %d < 1", cap);
    C2S_REQUIRE(from_logits == 0 || from_logits == 1, "parcel_soft_vote: from_logits is 0 or 1");
    C2S_REQUIRE(outside == 0 || outside == 1, "parcel_soft_vote: outside is 0 (zero) or 1 (keep)");
    C2S_REQUIRE(!(bg_mean != bg_mean), "parcel_soft_vote: bg_mean is NaN");
    const size_t need = c2s_parcel_soft_vote_workspace_bytes(B, cap, K);
    C2S_REQUIRE(need > 0, "parcel_soft_vote: B * cap * K = %ld entries are more than int indices reach", (long)B * cap * K);
    C2S_REQUIRE((uintptr_t)workspace % 16 == 0, "parcel_soft_vote: workspace not 16-byte aligned");
    C2S_REQUIRE(ws_bytes >= need, "parcel_soft_vote: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const int n = B * H * W, HW = H * W, np = B * cap;
    u64* S = (u64*)workspace;
    int* cnt = (int*)(S + (size_t)np * K);
    hipStream_t st = (hipStream_t)stream;
    const dim3 t(256), gsum((unsigned)((n + 256L * PS_ITER - 1) / (256L * PS_ITER)));
    hipLaunchKernelGGL(soft_zero_kernel, dim3(grid_for((long)(need / 4), PC_BLOCKS)), t, 0, st, (unsigned*)workspace, need / 4);
    C2S_CHECK_LAUNCH("soft_zero");
    if (K <= 4)
        hipLaunchKernelGGL(soft_sum_kernel<4>, gsum, t, 0, st, scores, labels, S, cnt, (long)n, HW, K, cap, from_logits, error);
    else if (K <= 8)
        hipLaunchKernelGGL(soft_sum_kernel<8>, gsum, t, 0, st, scores, labels, S, cnt, (long)n, HW, K, cap, from_logits, error);
    else if (K <= 16)
        hipLaunchKernelGGL(soft_sum_kernel<16>, gsum, t, 0, st, scores, labels, S, cnt, (long)n, HW, K, cap, from_logits, error);
    else
        hipLaunchKernelGGL(soft_sum_kernel<32>, gsum, t, 0, st, scores, labels, S, cnt, (long)n, HW, K, cap, from_logits, error);
    C2S_CHECK_LAUNCH("soft_sum");
    hipLaunchKernelGGL(soft_winner_kernel, dim3(grid_for(np, PC_BLOCKS)), t, 0, st, S, cnt, parcel_label, parcel_top2, parcel_mean,
                       parcel_pixels, np, K, bg_mean);
    C2S_CHECK_LAUNCH("soft_winner");
    hipLaunchKernelGGL(soft_write_kernel, dim3(grid_for(n, PC_BLOCKS)), t, 0, st, scores, labels, parcel_label, (int64_t*)out, n, HW, K, cap,
                       outside);
    C2S_CHECK_LAUNCH("soft_write");
    return C2S_OK;
}
