// The steps on either side of the hot path that move whole batches:
//
//  * c2s_collate_series : dataset __getitem__ tail + pad_collate as ONE pass from the raw patch series (host-pinned or
//    device memory) to the padded, normalised, band-reordered model input in HBM, plus the padded dates and the per-frame
//    flags.  Reference: src/datasets/s2_ts_cz_crop.py:366-374 (np.load(...).astype(float32)[:, channels_order]),
//    :393-398 ((d - mean[c]) / std[c], fp32), src/utils.py:14-32 (pad_tensor / pad_collate: zero frames appended up to
//    the longest series of the batch, for the data and for the dates), train.py:291 (band order [2,1,0,4,5,6,3,7,8,9]).
//  * c2s_softmax_stitch : tiled-inference tail, src/webapp/prediction.py:310-333: Softmax(dim=1) of every patch's logits,
//    top-1 class, the einops re-tiling '(h w) c h1 w1 -> c (h h1) (w w1)' and the crop to 1098 x 1098, written straight
//    into the tile rasters.
//  * c2s_cut_windows / c2s_softmax_blend / c2s_blend_finish : the same tail for a whole raster series predicted on
//    overlapping windows (inference.predict_raster; no counterpart in the reference): windows cut out of the series on the
//    device, their softmax blended into the raster with a taper by a per-pixel gather, normalised and arg-maxed in place.
//  * c2s_window_frames / c2s_cut_windows_raw : the same windows from the series as STORED (int16 / uint16 / float32):
//    which acquisitions each window keeps (empty ones, nodata in every band, dropped per window), then cut + collate in
//    one pass, so that no fp32 copy of the raster ever exists.
//
// Both are HBM/PCIe-bound byte movers (no reuse): the collate kernel reads each source element once with 16-byte lanes
// (8-byte for 16-bit sources) and writes 16-byte lanes; padding frames are written as zeros by the same grid.
#include "common.h"

namespace {

struct CollateParams {
    const void* src;            // concatenated series: [sum_b T_b][Cs][HW] in the dataset's storage type
    const long long* offsets;   // [B+1] frame offsets of the series inside src (device-accessible)
    const long long* src_dates; // [sum_b T_b] (device-accessible) or NULL
    float* x;                   // [B][T][C][HW]
    long long* dates;           // [B][T] or NULL
    int* valid;                 // [B*T] or NULL
    int B, T, C, Cs, HW;
    int order[16];              // output channel c reads source channel order[c]
    float mean[16], stdv[16];   // in OUTPUT channel order (reference norm_values, already re-ordered)
    int normalise;
    float pad_value;
    int ndvi_a, ndvi_b;         // >= 0: the LAST output channel is the NDVI of source channels (a, b), not normalised
};

// The ONE statement of the per-element arithmetic, shared by collate_kernel and cut_windows_raw_kernel.
// (d - mean) / std with IEEE fp32 subtraction and division, as torch evaluates it (no reciprocal, no fma)
__device__ __forceinline__ float normalised(float f, float m, float s) { return __fdiv_rn(__fsub_rn(f, m), s); }
// add_ndvi (s2_ts_cz_crop.py:376-391,401-402): (NIR - red) / (NIR + red) of the raw bands, 0 where the sum is 0 and where
// the quotient leaves [-1, 1]; appended after the normalised bands, itself not normalised.  IEEE fp32 add / sub / div.
__device__ __forceinline__ float ndvi_of(float a, float b) {
    const float sum = __fadd_rn(a, b);
    const float v = sum == 0.f ? 0.f : __fdiv_rn(__fsub_rn(a, b), sum);
    return (v < -1.f || v > 1.f) ? 0.f : v;
}

template <typename S> struct Vec4;
template <> struct Vec4<float> { using type = float4; };
template <> struct Vec4<short> { using type = short4; };
template <> struct Vec4<unsigned short> { using type = ushort4; };

// grid: (chunks of the HW plane, C, B*T).  Every thread converts 4 consecutive pixels.
template <typename S>
__global__ __launch_bounds__(256) void collate_kernel(CollateParams p) {
    const int n = blockIdx.z, c = blockIdx.y;
    const int b = n / p.T, t = n % p.T;
    const long long beg = p.offsets[b], len = p.offsets[b + 1] - beg;
    const bool real = t < len;
    if (c == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        if (p.valid) p.valid[n] = real ? 1 : 0;
        if (p.dates) p.dates[n] = (real && p.src_dates) ? p.src_dates[beg + t] : 0;       // dates are padded with 0 too
    }
    float4* out = reinterpret_cast<float4*>(p.x + ((size_t)n * p.C + c) * p.HW);
    const int q = p.HW >> 2;
    if (!real) {
        const float4 z = make_float4(p.pad_value, p.pad_value, p.pad_value, p.pad_value);
        for (int i = blockIdx.x * 256 + threadIdx.x; i < q; i += gridDim.x * 256) out[i] = z;
        return;
    }
    using V = typename Vec4<S>::type;
    if (p.ndvi_a >= 0 && c == p.C - 1) {
        const V* ia = reinterpret_cast<const V*>(static_cast<const S*>(p.src) + ((size_t)(beg + t) * p.Cs + p.ndvi_a) * p.HW);
        const V* ib = reinterpret_cast<const V*>(static_cast<const S*>(p.src) + ((size_t)(beg + t) * p.Cs + p.ndvi_b) * p.HW);
        for (int i = blockIdx.x * 256 + threadIdx.x; i < q; i += gridDim.x * 256) {
            const V va = ia[i], vb = ib[i];
            const float a4[4] = {(float)va.x, (float)va.y, (float)va.z, (float)va.w};
            const float b4[4] = {(float)vb.x, (float)vb.y, (float)vb.z, (float)vb.w};
            out[i] = make_float4(ndvi_of(a4[0], b4[0]), ndvi_of(a4[1], b4[1]), ndvi_of(a4[2], b4[2]), ndvi_of(a4[3], b4[3]));
        }
        return;
    }
    const V* in = reinterpret_cast<const V*>(static_cast<const S*>(p.src) + ((size_t)(beg + t) * p.Cs + p.order[c]) * p.HW);
    const float m = p.mean[c], s = p.stdv[c];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < q; i += gridDim.x * 256) {
        const V v = in[i];
        float4 f = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);      // .astype(np.float32): exact for 16-bit ints
        if (p.normalise) {
            f.x = normalised(f.x, m, s);
            f.y = normalised(f.y, m, s);
            f.z = normalised(f.z, m, s);
            f.w = normalised(f.w, m, s);
        }
        out[i] = f;
    }
}

// One thread per output pixel of the cropped raster: reads the K logits of its patch pixel once, writes K probabilities.
__global__ __launch_bounds__(256) void softmax_stitch_kernel(const float* __restrict__ logits, float* __restrict__ proba,
                                                             long long* __restrict__ top1, int first_patch, int npatch,
                                                             int K, int ph, int pw, int grid_w, int out_h, int out_w) {
    const long total = (long)npatch * ph * pw;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int x1 = (int)(e % pw), y1 = (int)((e / pw) % ph), pi = (int)(e / ((long)pw * ph));
        const int patch = first_patch + pi;
        const int oy = (patch / grid_w) * ph + y1, ox = (patch % grid_w) * pw + x1;
        if (oy >= out_h || ox >= out_w) continue;                                      // the crop (prediction.py:330-331)
        const float* lp = logits + ((size_t)pi * K * ph + y1) * pw + x1;
        const size_t cs = (size_t)ph * pw;
        float mx = lp[0];
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, lp[k * cs]);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += expf(lp[k * cs] - mx);
        const size_t os = (size_t)out_h * out_w;
        float* op = proba + (size_t)oy * out_w + ox;
        // top-1 = first maximum of the PROBABILITIES (pred_.max(dim=1)[1], prediction.py:316): logits closer than one
        // ulp of exp() tie there and resolve to the lower class, as in the reference
        float best = -1.f;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const float pk = expf(lp[k * cs] - mx) / s;
            op[k * os] = pk;
            if (pk > best) { best = pk; arg = k; }
        }
        if (top1) top1[(size_t)oy * out_w + ox] = arg;
    }
}

// ---------------------------------------------------------------- overlapped sliding windows over a whole raster
// Window placement along one axis (include/c2s_hip.h): the ONE statement of it, used by the exported host functions, by
// the launch code and by the kernels.
__host__ __device__ __forceinline__ int win_count(int size, int patch, int stride) {
    return size <= patch ? 1 : (size - patch + stride - 1) / stride + 1;
}
__host__ __device__ __forceinline__ int win_origin(int i, int size, int patch, int stride) {
    const long long o = (long long)i * stride, last = size > patch ? size - patch : 0;
    return (int)(o < last ? o : last);                                  // the last window is clamped to the raster edge
}

struct CutParams {
    const float* series;        // [T][C][H][W]
    float* x;                   // [nwin][T][C][ph][pw]
    int T, C, H, W, ph, pw, sy, sx, nx, first, nwin, flip;
    float fill[16];             // per channel, where the raster is smaller than a window
};

// Every thread writes 4 consecutive pixels of a window row (one 16-byte store: pw % 8 == 0) from 4 dword loads: a raster
// row starts at any 4-byte boundary, and under flip & 1 the lanes read their row backwards.  Grid-stride over the quads.
__global__ __launch_bounds__(256) void cut_windows_kernel(CutParams p) {
    const int qw = p.pw >> 2;
    const size_t total = (size_t)p.nwin * p.T * p.C * p.ph * qw;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        size_t r = e;
        const int xq = (int)(r % qw); r /= qw;
        const int y1 = (int)(r % p.ph); r /= p.ph;
        const int c = (int)(r % p.C); r /= p.C;
        const int t = (int)(r % p.T);
        const int w = p.first + (int)(r / p.T);
        const int oy = win_origin(w / p.nx, p.H, p.ph, p.sy), ox = win_origin(w % p.nx, p.W, p.pw, p.sx);
        const int sy = oy + ((p.flip & 2) ? p.ph - 1 - y1 : y1);
        const float fv = p.fill[c];
        float o[4] = {fv, fv, fv, fv};
        if (sy < p.H) {
            const float* row = p.series + (((size_t)t * p.C + c) * p.H + sy) * p.W;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x1 = xq * 4 + j;
                const int sx = ox + ((p.flip & 1) ? p.pw - 1 - x1 : x1);
                if (sx < p.W) o[j] = row[sx];
            }
        }
        reinterpret_cast<float4*>(p.x)[e] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---------------------------------------------------------------- the same windows from the STORED series
// Which frames a window keeps.  Count: one workgroup per (window, frame) over the window's pixels INSIDE the raster; a
// pixel is empty when every source channel equals nodata.  (float)v is exact for the 16-bit types, so the comparison is
// the integer one.  Channel 0 decides for almost every pixel of real data; the others are read only behind it.  Integer
// sums: the result does not depend on the order, hence not on the launch geometry.
struct FramesParams {
    const void* src;            // [T][Cs][H][W]
    const long long* dates;     // [T]
    int* nodata_px;             // [nwin][T]
    int* slots;                 // [nwin][T]
    int* counts;                // [nwin]
    long long* win_dates;       // [nwin][T]
    int T, Cs, H, W, ph, pw, sy, sx, nx, first, nwin, permille;
    float nodata;
};

template <typename S>
__global__ __launch_bounds__(256) void count_nodata_kernel(FramesParams p) {
    __shared__ int part[4];
    const int wi = blockIdx.x / p.T, t = blockIdx.x % p.T;
    const int w = p.first + wi;
    const int oy = win_origin(w / p.nx, p.H, p.ph, p.sy), ox = win_origin(w % p.nx, p.W, p.pw, p.sx);
    const int h = min(p.ph, p.H - oy), wd = min(p.pw, p.W - ox);
    const size_t plane = (size_t)p.H * p.W;
    const S* f0 = static_cast<const S*>(p.src) + (size_t)t * p.Cs * plane;
    int n = 0;
    for (int i = threadIdx.x; i < h * wd; i += 256) {
        const size_t at = (size_t)(oy + i / wd) * p.W + (ox + i % wd);
        bool empty = (float)f0[at] == p.nodata;
        for (int cs = 1; empty && cs < p.Cs; ++cs) empty = (float)f0[cs * plane + at] == p.nodata;
        n += empty ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) p.nodata_px[(size_t)wi * p.T + t] = part[0] + part[1] + part[2] + part[3];
}

// Ordered compaction: one wave (one workgroup of 64 lanes) per window walks T in chunks of 64; ballot + popcount place
// the kept frames in ascending t.  A window that would keep none keeps the frame with the fewest empty pixels, lowest t
// on a tie: the smallest (nodata_px, t) key.
__global__ __launch_bounds__(64) void compact_frames_kernel(FramesParams p) {
    const int wi = blockIdx.x, lane = threadIdx.x;
    const int w = p.first + wi;
    const int oy = win_origin(w / p.nx, p.H, p.ph, p.sy), ox = win_origin(w % p.nx, p.W, p.pw, p.sx);
    const long long inside = (long long)min(p.ph, p.H - oy) * min(p.pw, p.W - ox);
    const int* px = p.nodata_px + (size_t)wi * p.T;
    int* slots = p.slots + (size_t)wi * p.T;
    long long* wd = p.win_dates + (size_t)wi * p.T;
    int count = 0;
    long long best = 0x7fffffffffffffffLL;
    for (int base = 0; base < p.T; base += 64) {
        const int t = base + lane;
        const int n = t < p.T ? px[t] : 0;
        const bool keep = t < p.T && 1000LL * n <= (long long)p.permille * inside;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int j = count + (int)__popcll(mask & ((1ULL << lane) - 1ULL));
            slots[j] = t;
            wd[j] = p.dates[t];
        }
        count += (int)__popcll(mask);
        if (t < p.T) best = min(best, ((long long)n << 32) | t);
    }
    if (count == 0) {                                                   // uniform: count comes from ballots
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        const int t = (int)(best & 0xffffffffLL);
        if (lane == 0) { slots[0] = t; wd[0] = p.dates[t]; }
        count = 1;
    }
    for (int j = count + lane; j < p.T; j += 64) { slots[j] = -1; wd[j] = 0; }     // pad_collate's layout
    if (lane == 0) p.counts[wi] = count;
}

struct CutRawParams {
    const void* src;            // [T][Cs][H][W] in the storage type
    float* x;                   // [nwin][T][C][ph][pw]
    const int* slots;           // [nwin][T] or NULL
    int T, C, Cs, H, W, ph, pw, sy, sx, nx, first, nwin, flip;
    int order[16];              // output channel c reads source channel order[c]
    float mean[16], stdv[16], fill[16];
    int normalise;
    float pad_value;
    int ndvi_a, ndvi_b;         // >= 0: the LAST output channel is the NDVI of source channels (a, b), not normalised
};

// Four consecutive stored elements.  16-bit: two dword loads where the address is 4-byte aligned, else element, dword,
// element -- the address itself decides, and exactly the four elements are read either way.
template <typename S>
__device__ __forceinline__ void load4(const S* q, S v[4]) {
    if constexpr (sizeof(S) == 2) {
        if ((reinterpret_cast<uintptr_t>(q) & 3) == 0) {
            const unsigned a = *reinterpret_cast<const unsigned*>(q), b = *reinterpret_cast<const unsigned*>(q + 2);
            v[0] = (S)(a & 0xffffu); v[1] = (S)(a >> 16); v[2] = (S)(b & 0xffffu); v[3] = (S)(b >> 16);
        } else {
            const unsigned b = *reinterpret_cast<const unsigned*>(q + 1);
            v[0] = q[0]; v[1] = (S)(b & 0xffffu); v[2] = (S)(b >> 16); v[3] = q[3];
        }
    } else {
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    }
}

// cut_windows_kernel's work on the stored series: every thread writes 4 consecutive pixels of a window row (one 16-byte
// store) from its 4 source elements -- a 16-bit raster row starts at any 2-byte boundary (odd W, any ox), so load4 widens
// per address (1.9 ms against 2.85 ms with four element loads for the 144 windows of a 1098^2, T = 60 raster, even and odd
// widths alike: profiles/raster_raw_bench.txt); a quad that reaches past the raster goes element by element.
// Grid (quads of one window plane, C, output frames): the frame, its slot, the window origin and
// the channel's constants are uniform over a workgroup, and a thread's own index arithmetic is 32-bit.  Output frame j of
// a window is source frame slots[w][j]; a slot of -1 is pad_value.
template <typename S>
__global__ __launch_bounds__(256) void cut_windows_raw_kernel(CutRawParams p) {
    const int qw = p.pw >> 2, quads = p.ph * qw, c = blockIdx.y;
    const size_t plane = (size_t)p.H * p.W;
    const bool ndvi = p.ndvi_a >= 0 && c == p.C - 1;
    const int ca = ndvi ? p.ndvi_a : p.order[c], cb = ndvi ? p.ndvi_b : 0;
    const float fv = p.fill[c], m = p.mean[c], sd = p.stdv[c];
    for (int f = blockIdx.z; f < p.nwin * p.T; f += gridDim.z) {        // f = wi * T + j
        const int wi = f / p.T, w = p.first + wi;
        const int s = p.slots ? p.slots[f] : f - wi * p.T;
        float4* out = reinterpret_cast<float4*>(p.x) + ((size_t)f * p.C + c) * quads;
        if (s < 0 || s >= p.T) {
            const float4 pad = make_float4(p.pad_value, p.pad_value, p.pad_value, p.pad_value);
            for (int i = blockIdx.x * 256 + threadIdx.x; i < quads; i += gridDim.x * 256) out[i] = pad;
            continue;
        }
        const int oy = win_origin(w / p.nx, p.H, p.ph, p.sy), ox = win_origin(w % p.nx, p.W, p.pw, p.sx);
        const S* fa = static_cast<const S*>(p.src) + ((size_t)s * p.Cs + ca) * plane;
        const S* fb = static_cast<const S*>(p.src) + ((size_t)s * p.Cs + cb) * plane;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < quads; i += gridDim.x * 256) {
            const int y1 = i / qw, xq = i - y1 * qw;
            const int sy = oy + ((p.flip & 2) ? p.ph - 1 - y1 : y1);
            const size_t row = (size_t)sy * p.W;
            float o[4];
            const int lo = ox + ((p.flip & 1) ? p.pw - 4 - xq * 4 : xq * 4);   // leftmost of the 4 source columns
            if (sy < p.H && lo + 3 < p.W) {
                S va[4], vb[4];
                load4(fa + row + lo, va);
                if (ndvi) load4(fb + row + lo, vb);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int kk = (p.flip & 1) ? 3 - k : k;
                    const float a = (float)va[kk];
                    o[k] = ndvi ? ndvi_of(a, (float)vb[kk]) : (p.normalise ? normalised(a, m, sd) : a);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x1 = xq * 4 + k;
                    const int sx = ox + ((p.flip & 1) ? p.pw - 1 - x1 : x1);
                    float v = fv;
                    if (sy < p.H && sx < p.W) {
                        const float a = (float)fa[row + sx];            // .astype(np.float32): exact for 16-bit ints
                        v = ndvi ? ndvi_of(a, (float)fb[row + sx]) : (p.normalise ? normalised(a, m, sd) : a);
                    }
                    o[k] = v;
                }
            }
            out[i] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// Gather: one thread owns one raster pixel of the rows [y0, y0 + rows) that the batch's windows touch, and visits the
// covering windows of [first, first + nwin) in ascending index; the softmax arithmetic is softmax_stitch_kernel's.  The K
// running sums live in registers (KMAX: the instantiation that holds K); __fmul_rn / __fadd_rn keep the sum one fixed
// left-to-right expression of separate multiplies and adds.
template <int KMAX>
__global__ __launch_bounds__(256) void softmax_blend_kernel(const float* __restrict__ logits, float* __restrict__ acc,
                                                            float* __restrict__ wsum, const float* __restrict__ ty,
                                                            const float* __restrict__ tx, int first, int nwin, int K, int ph,
                                                            int pw, int H, int W, int sy, int sx, int flip, int ny, int nx,
                                                            int y0, int rows) {
    const size_t total = (size_t)rows * W, hw = (size_t)H * W, cs = (size_t)ph * pw;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int y = y0 + (int)(e / W), x = (int)(e % W);
        const size_t pix = (size_t)y * W + x;
        // unclamped window i covers y iff i * stride <= y < i * stride + patch; the clamped last window lies lower, never
        // below its neighbour, so the scan starts at the first unclamped candidate and stops at the first origin past y
        const int iy0 = y >= ph ? (y - ph) / sy + 1 : 0, ix0 = x >= pw ? (x - pw) / sx + 1 : 0;
        float a[KMAX];
        float ws = 0.f;
        bool any = false;
        for (int iy = iy0; iy < ny; ++iy) {
            const int oy = win_origin(iy, H, ph, sy);
            if (oy > y) break;
            if (y - oy >= ph) continue;
            for (int ix = ix0; ix < nx; ++ix) {
                const int ox = win_origin(ix, W, pw, sx);
                if (ox > x) break;
                if (x - ox >= pw) continue;
                const int wi = iy * nx + ix - first;
                if (wi < 0 || wi >= nwin) continue;
                if (!any) {
                    any = true;
                    ws = wsum[pix];
#pragma unroll
                    for (int k = 0; k < KMAX; ++k)
                        if (k < K) a[k] = acc[k * hw + pix];
                }
                const int y1 = y - oy, x1 = x - ox;
                const int ly = (flip & 2) ? ph - 1 - y1 : y1, lx = (flip & 1) ? pw - 1 - x1 : x1;   // un-mirror the pass
                const float* lp = logits + ((size_t)wi * K * ph + ly) * pw + lx;
                float l[KMAX];
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) l[k] = lp[k * cs];
                float mx = l[0];
#pragma unroll
                for (int k = 1; k < KMAX; ++k)
                    if (k < K) mx = fmaxf(mx, l[k]);
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) s += expf(l[k] - mx);
                const float w = (ty || tx) ? __fmul_rn(ty ? ty[y1] : 1.f, tx ? tx[x1] : 1.f) : 1.f;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) a[k] = __fadd_rn(a[k], __fmul_rn(w, expf(l[k] - mx) / s));
                ws = __fadd_rn(ws, w);
            }
        }
        if (!any) continue;                                             // no window of this batch covers the pixel
        wsum[pix] = ws;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) acc[k * hw + pix] = a[k];
    }
}

// acc / wsum in place (IEEE divide) and the first maximum of the probabilities, as softmax_stitch_kernel picks it.
__global__ __launch_bounds__(256) void blend_finish_kernel(float* __restrict__ acc, const float* __restrict__ wsum,
                                                           long long* __restrict__ top1, int K, size_t hw) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < hw; e += (size_t)gridDim.x * 256) {
        const float s = wsum[e];
        float best = -1.f;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const float pk = __fdiv_rn(acc[k * hw + e], s);
            acc[k * hw + e] = pk;
            if (pk > best) { best = pk; arg = k; }
        }
        if (top1) top1[e] = arg;
    }
}

int mover_blocks(size_t items) {
    size_t b = (items + 255) / 256;
    return (int)(b > 2048 ? 2048 : (b ? b : 1));
}

bool window_args_ok(int size, int patch, int stride) { return size >= 1 && patch >= 1 && stride >= 1 && stride <= patch; }

}  // namespace

extern "C" int c2s_window_count(int size, int patch, int stride) {
    C2S_REQUIRE(window_args_ok(size, patch, stride), "window_count: need size >= 1 and 1 <= stride <= patch");
    return win_count(size, patch, stride);
}

extern "C" int c2s_window_origin(int i, int size, int patch, int stride) {
    C2S_REQUIRE(window_args_ok(size, patch, stride), "window_origin: need size >= 1 and 1 <= stride <= patch");
    C2S_REQUIRE(i >= 0 && i < win_count(size, patch, stride), "window_origin: window index %d out of range", i);
    return win_origin(i, size, patch, stride);
}

extern "C" int c2s_cut_windows(const float* series, float* x, int T, int C, int H, int W, int ph, int pw, int stride_y,
                               int stride_x, int first_window, int nwin, int flip, const float* host_fill, void* stream) {
    C2S_REQUIRE(series && x, "cut_windows: null pointer");
    C2S_REQUIRE(T > 0 && C > 0 && C <= 16 && H > 0 && W > 0, "cut_windows: bad shape (T, H, W >= 1, 1 <= C <= 16)");
    C2S_REQUIRE(ph >= 16 && pw >= 16 && ph % 8 == 0 && pw % 8 == 0, "cut_windows: window sides must be multiples of 8, >= 16");
    C2S_REQUIRE(stride_y >= 1 && stride_y <= ph && stride_x >= 1 && stride_x <= pw, "cut_windows: need 1 <= stride <= patch");
    C2S_REQUIRE(flip >= 0 && flip <= 3, "cut_windows: flip is a mask of 1 (x) and 2 (y)");
    const int ny = win_count(H, ph, stride_y), nx = win_count(W, pw, stride_x);
    C2S_REQUIRE(first_window >= 0 && nwin > 0 && (long long)first_window + nwin <= (long long)ny * nx,
                "cut_windows: windows [%d, %d + %d) outside the %d x %d grid", first_window, first_window, nwin, ny, nx);
    CutParams p = {};
    p.series = series; p.x = x; p.T = T; p.C = C; p.H = H; p.W = W; p.ph = ph; p.pw = pw; p.sy = stride_y; p.sx = stride_x;
    p.nx = nx; p.first = first_window; p.nwin = nwin; p.flip = flip;
    for (int c = 0; c < C; ++c) p.fill[c] = host_fill ? host_fill[c] : 0.f;
    const size_t quads = (size_t)nwin * T * C * ph * (pw / 4);
    hipLaunchKernelGGL(cut_windows_kernel, dim3(mover_blocks(quads)), dim3(256), 0, (hipStream_t)stream, p);
    C2S_CHECK_LAUNCH("cut_windows");
    return C2S_OK;
}

extern "C" int c2s_window_frames(const void* src, int src_dtype, const long long* dates, int* nodata_px, int* slots, int* counts,
                                 long long* win_dates, int T, int Cs, int H, int W, int ph, int pw, int stride_y, int stride_x,
                                 int first_window, int nwin, float nodata, int max_nodata_permille, void* stream) {
    C2S_REQUIRE(src && dates && nodata_px && slots && counts && win_dates, "window_frames: null pointer");
    C2S_REQUIRE(src_dtype == C2S_SRC_F32 || src_dtype == C2S_SRC_I16 || src_dtype == C2S_SRC_U16, "window_frames: unknown src_dtype %d", src_dtype);
    C2S_REQUIRE(((uintptr_t)src & (src_dtype == C2S_SRC_F32 ? 3 : 1)) == 0, "window_frames: src is not aligned to its element size");
    C2S_REQUIRE(T > 0 && Cs > 0 && H > 0 && W > 0, "window_frames: bad shape (T, Cs, H, W >= 1)");
    C2S_REQUIRE(ph >= 16 && pw >= 16 && ph % 8 == 0 && pw % 8 == 0 && (long long)ph * pw < (1LL << 30),
                "window_frames: window sides must be multiples of 8, >= 16");
    C2S_REQUIRE(stride_y >= 1 && stride_y <= ph && stride_x >= 1 && stride_x <= pw, "window_frames: need 1 <= stride <= patch");
    C2S_REQUIRE(max_nodata_permille >= 0 && max_nodata_permille <= 1000, "window_frames: max_nodata_permille is in 0 .. 1000, got %d", max_nodata_permille);
    const int ny = win_count(H, ph, stride_y), nx = win_count(W, pw, stride_x);
    C2S_REQUIRE(first_window >= 0 && nwin > 0 && (long long)first_window + nwin <= (long long)ny * nx,
                "window_frames: windows [%d, %d + %d) outside the %d x %d grid", first_window, first_window, nwin, ny, nx);
    C2S_REQUIRE((long long)nwin * T < (1LL << 31), "window_frames: nwin * T must stay below 2^31 for one launch");
    FramesParams p = {};
    p.src = src; p.dates = dates; p.nodata_px = nodata_px; p.slots = slots; p.counts = counts; p.win_dates = win_dates;
    p.T = T; p.Cs = Cs; p.H = H; p.W = W; p.ph = ph; p.pw = pw; p.sy = stride_y; p.sx = stride_x; p.nx = nx;
    p.first = first_window; p.nwin = nwin; p.permille = max_nodata_permille; p.nodata = nodata;
    const dim3 grid((unsigned)((long long)nwin * T)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (src_dtype) {
        case C2S_SRC_F32: hipLaunchKernelGGL(count_nodata_kernel<float>, grid, block, 0, st, p); break;
        case C2S_SRC_I16: hipLaunchKernelGGL(count_nodata_kernel<short>, grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL(count_nodata_kernel<unsigned short>, grid, block, 0, st, p); break;
    }
    C2S_CHECK_LAUNCH("window_frames (count)");
    hipLaunchKernelGGL(compact_frames_kernel, dim3(nwin), dim3(64), 0, st, p);
    C2S_CHECK_LAUNCH("window_frames (compact)");
    return C2S_OK;
}

extern "C" int c2s_cut_windows_raw(const void* src, int src_dtype, float* x, const int* slots, int T, int C, int Cs, int H, int W,
                                   int ph, int pw, int stride_y, int stride_x, int first_window, int nwin, int flip,
                                   const int* host_channel_order, const float* host_mean, const float* host_std,
                                   const float* host_fill, float pad_value, int ndvi_a, int ndvi_b, void* stream) {
    C2S_REQUIRE(src && x, "cut_windows_raw: null pointer");
    C2S_REQUIRE(src_dtype == C2S_SRC_F32 || src_dtype == C2S_SRC_I16 || src_dtype == C2S_SRC_U16, "cut_windows_raw: unknown src_dtype %d", src_dtype);
    C2S_REQUIRE(((uintptr_t)src & (src_dtype == C2S_SRC_F32 ? 3 : 1)) == 0, "cut_windows_raw: src is not aligned to its element size");
    const bool ndvi = ndvi_a >= 0 || ndvi_b >= 0;
    C2S_REQUIRE(T > 0 && C > 0 && C <= 16 && Cs > 0 && H > 0 && W > 0, "cut_windows_raw: bad shape (T, Cs, H, W >= 1, 1 <= C <= 16)");
    C2S_REQUIRE(!ndvi || (ndvi_a >= 0 && ndvi_a < Cs && ndvi_b >= 0 && ndvi_b < Cs && C >= 2), "cut_windows_raw: NDVI source channels out of range");
    C2S_REQUIRE(ph >= 16 && pw >= 16 && ph % 8 == 0 && pw % 8 == 0 && (long long)ph * pw < (1LL << 30),
                "cut_windows_raw: window sides must be multiples of 8, >= 16");
    C2S_REQUIRE(stride_y >= 1 && stride_y <= ph && stride_x >= 1 && stride_x <= pw, "cut_windows_raw: need 1 <= stride <= patch");
    C2S_REQUIRE(flip >= 0 && flip <= 3, "cut_windows_raw: flip is a mask of 1 (x) and 2 (y)");
    C2S_REQUIRE((host_mean == nullptr) == (host_std == nullptr), "cut_windows_raw: mean and std come together");
    const int ny = win_count(H, ph, stride_y), nx = win_count(W, pw, stride_x);
    C2S_REQUIRE(first_window >= 0 && nwin > 0 && (long long)first_window + nwin <= (long long)ny * nx,
                "cut_windows_raw: windows [%d, %d + %d) outside the %d x %d grid", first_window, first_window, nwin, ny, nx);
    C2S_REQUIRE((long long)nwin * T < (1LL << 31), "cut_windows_raw: nwin * T must stay below 2^31 for one launch");
    CutRawParams p = {};
    p.src = src; p.x = x; p.slots = slots; p.T = T; p.C = C; p.Cs = Cs; p.H = H; p.W = W; p.ph = ph; p.pw = pw;
    p.sy = stride_y; p.sx = stride_x; p.nx = nx; p.first = first_window; p.nwin = nwin; p.flip = flip;
    p.normalise = host_mean != nullptr; p.pad_value = pad_value;
    p.ndvi_a = ndvi ? ndvi_a : -1; p.ndvi_b = ndvi ? ndvi_b : -1;
    for (int c = 0; c < C; ++c) {
        p.fill[c] = host_fill ? host_fill[c] : 0.f;
        p.stdv[c] = 1.f;
        if (ndvi && c == C - 1) continue;                               // the NDVI channel has no order / mean / std entry
        p.order[c] = host_channel_order ? host_channel_order[c] : c;
        C2S_REQUIRE(p.order[c] >= 0 && p.order[c] < Cs, "cut_windows_raw: channel_order entry out of range (0 .. Cs - 1)");
        p.mean[c] = host_mean ? host_mean[c] : 0.f;
        p.stdv[c] = host_std ? host_std[c] : 1.f;
    }
    const int frames = nwin * T, xblocks = cdiv(ph * (pw / 4), 256);
    const dim3 grid(xblocks > 4 ? 4 : xblocks, C, frames > 65535 ? 65535 : frames), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (src_dtype) {
        case C2S_SRC_F32: hipLaunchKernelGGL(cut_windows_raw_kernel<float>, grid, block, 0, st, p); break;
        case C2S_SRC_I16: hipLaunchKernelGGL(cut_windows_raw_kernel<short>, grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL(cut_windows_raw_kernel<unsigned short>, grid, block, 0, st, p); break;
    }
    C2S_CHECK_LAUNCH("cut_windows_raw");
    return C2S_OK;
}

extern "C" int c2s_softmax_blend(const float* logits, float* acc, float* wsum, const float* wy, const float* wx,
                                 int first_window, int nwin, int K, int ph, int pw, int H, int W, int stride_y, int stride_x,
                                 int flip, void* stream) {
    C2S_REQUIRE(logits && acc && wsum, "softmax_blend: null pointer");
    C2S_REQUIRE(K >= 1 && K <= 32, "softmax_blend: need 1 <= K <= 32");
    C2S_REQUIRE(ph > 0 && pw > 0 && H > 0 && W > 0, "softmax_blend: bad shape");
    C2S_REQUIRE(stride_y >= 1 && stride_y <= ph && stride_x >= 1 && stride_x <= pw, "softmax_blend: need 1 <= stride <= patch");
    C2S_REQUIRE(flip >= 0 && flip <= 3, "softmax_blend: flip is a mask of 1 (x) and 2 (y)");
    const int ny = win_count(H, ph, stride_y), nx = win_count(W, pw, stride_x);
    C2S_REQUIRE(first_window >= 0 && nwin > 0 && (long long)first_window + nwin <= (long long)ny * nx,
                "softmax_blend: windows [%d, %d + %d) outside the %d x %d grid", first_window, first_window, nwin, ny, nx);
    const int y0 = win_origin(first_window / nx, H, ph, stride_y);
    int y1 = win_origin((first_window + nwin - 1) / nx, H, ph, stride_y) + ph;
    if (y1 > H) y1 = H;
    const int rows = y1 - y0;
    const dim3 grid(mover_blocks((size_t)rows * W)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define C2S_BLEND(KM)                                                                                                     \
    hipLaunchKernelGGL(softmax_blend_kernel<KM>, grid, block, 0, st, logits, acc, wsum, wy, wx, first_window, nwin, K, ph, \
                       pw, H, W, stride_y, stride_x, flip, ny, nx, y0, rows)
    if (K <= 8) C2S_BLEND(8);
    else if (K <= 16) C2S_BLEND(16);
    else if (K <= 24) C2S_BLEND(24);
    else C2S_BLEND(32);
#undef C2S_BLEND
    C2S_CHECK_LAUNCH("softmax_blend");
    return C2S_OK;
}

extern "C" int c2s_blend_finish(float* acc_proba, const float* wsum, long long* top1, int K, int H, int W, void* stream) {
    C2S_REQUIRE(acc_proba && wsum, "blend_finish: null pointer");
    C2S_REQUIRE(K >= 1 && H > 0 && W > 0, "blend_finish: bad shape");
    const size_t hw = (size_t)H * W;
    hipLaunchKernelGGL(blend_finish_kernel, dim3(mover_blocks(hw)), dim3(256), 0, (hipStream_t)stream, acc_proba, wsum, top1, K, hw);
    C2S_CHECK_LAUNCH("blend_finish");
    return C2S_OK;
}

extern "C" int c2s_collate_series(const void* src, int src_dtype, const long long* offsets, const long long* src_dates,
                                  float* x, long long* dates, int* valid, int B, int T, int C, int Cs, int HW,
                                  const int* host_channel_order, const float* host_mean, const float* host_std,
                                  float pad_value, void* stream) {
    return c2s_collate_series_ndvi(src, src_dtype, offsets, src_dates, x, dates, valid, B, T, C, Cs, HW, host_channel_order,
                                   host_mean, host_std, pad_value, -1, -1, stream);
}

extern "C" int c2s_collate_series_ndvi(const void* src, int src_dtype, const long long* offsets, const long long* src_dates,
                                       float* x, long long* dates, int* valid, int B, int T, int C, int Cs, int HW,
                                       const int* host_channel_order, const float* host_mean, const float* host_std,
                                       float pad_value, int ndvi_a, int ndvi_b, void* stream) {
    C2S_REQUIRE(src && offsets && x, "collate_series: null pointer");
    const bool ndvi = ndvi_a >= 0 || ndvi_b >= 0;
    C2S_REQUIRE(!ndvi || (ndvi_a >= 0 && ndvi_a < Cs && ndvi_b >= 0 && ndvi_b < Cs && C >= 2), "collate_series: NDVI source channels out of range");
    C2S_REQUIRE(B > 0 && T > 0 && C > 0 && C <= 16 && Cs >= C - (ndvi ? 1 : 0) && HW > 0 && HW % 4 == 0, "collate_series: bad shape (C <= 16, HW %% 4 == 0)");
    C2S_REQUIRE((long)B * T < 65536 && C < 65536, "collate_series: too many frames for one launch");
    C2S_REQUIRE((host_mean == nullptr) == (host_std == nullptr), "collate_series: mean and std come together");
    CollateParams p = {};
    p.src = src; p.offsets = offsets; p.src_dates = src_dates; p.x = x; p.dates = dates; p.valid = valid;
    p.B = B; p.T = T; p.C = C; p.Cs = Cs; p.HW = HW; p.pad_value = pad_value;
    p.normalise = host_mean != nullptr;
    p.ndvi_a = ndvi ? ndvi_a : -1; p.ndvi_b = ndvi ? ndvi_b : -1;
    for (int c = 0; c < C - (ndvi ? 1 : 0); ++c) {
        p.order[c] = host_channel_order ? host_channel_order[c] : c;
        C2S_REQUIRE(p.order[c] >= 0 && p.order[c] < Cs, "collate_series: channel_order entry out of range");
        p.mean[c] = host_mean ? host_mean[c] : 0.f;
        p.stdv[c] = host_std ? host_std[c] : 1.f;
    }
    int chunks = (HW / 4 + 255) / 256;
    if (chunks > 16) chunks = 16;
    dim3 grid(chunks, C, B * T);
    hipStream_t st = (hipStream_t)stream;
    switch (src_dtype) {
        case C2S_SRC_F32: hipLaunchKernelGGL(collate_kernel<float>, grid, dim3(256), 0, st, p); break;
        case C2S_SRC_I16: hipLaunchKernelGGL(collate_kernel<short>, grid, dim3(256), 0, st, p); break;
        case C2S_SRC_U16: hipLaunchKernelGGL(collate_kernel<unsigned short>, grid, dim3(256), 0, st, p); break;
        default: c2s_set_error("collate_series: unknown src_dtype %d", src_dtype); return C2S_EINVAL;
    }
    C2S_CHECK_LAUNCH("collate_series");
    return C2S_OK;
}

extern "C" int c2s_softmax_stitch(const float* logits, float* proba, long long* top1, int first_patch, int npatch, int K,
                                  int ph, int pw, int grid_w, int out_h, int out_w, void* stream) {
    C2S_REQUIRE(logits && proba, "softmax_stitch: null pointer");
    C2S_REQUIRE(first_patch >= 0 && npatch > 0 && K > 0 && ph > 0 && pw > 0 && grid_w > 0 && out_h > 0 && out_w > 0,
                "softmax_stitch: bad shape");
    const long total = (long)npatch * ph * pw;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(softmax_stitch_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, logits, proba, top1,
                       first_patch, npatch, K, ph, pw, grid_w, out_h, out_w);
    C2S_CHECK_LAUNCH("softmax_stitch");
    return C2S_OK;
}
