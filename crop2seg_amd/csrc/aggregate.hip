// Attention-weighted temporal aggregation of skip feature maps (mode att_group), forward and backward.
// Reference: src/backbones/temporal_aggregator.py:14-45,58-70 -- nn.Upsample(bilinear, align_corners=False)
// of the attention masks, x.chunk(n_head) * attn, sum over T -- which materialises [B,T,C,H,W] products.
// Here the 4-tap bilinear weights are computed once per thread and x is streamed exactly once (HBM-bound).
#include "common.h"

namespace {

struct Taps {
    int i0, i1;
    float w0, w1;
};
// torch area_pixel_compute_source_index (align_corners=False)
__device__ __forceinline__ Taps taps_for(int dst, int in, int out) {
    Taps t;
    if (in == out) { t.i0 = dst; t.i1 = dst; t.w0 = 1.f; t.w1 = 0.f; return t; }
    if (in == 1) { t.i0 = 0; t.i1 = 0; t.w0 = 1.f; t.w1 = 0.f; return t; }        // one weight per plane (mode "mean")
    const float scale = (float)in / (float)out;
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.w1 = src - (float)t.i0;
    t.w0 = 1.f - t.w1;
    return t;
}

template <int CPG>
__global__ __launch_bounds__(256) void agg_fwd_kernel(const float* __restrict__ x, const float* __restrict__ attn,
                                                      const int* __restrict__ valid, float* __restrict__ out,
                                                      c2s_agg_desc d) {
    const long total = (long)d.B * d.n_head * d.H * d.W;
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int X = (int)(e % d.W);
    long r = e / d.W;
    const int Y = (int)(r % d.H); r /= d.H;
    const int g = (int)(r % d.n_head), b = (int)(r / d.n_head);
    const Taps ty = taps_for(Y, d.h, d.H), tx = taps_for(X, d.w, d.W);
    const size_t HW = (size_t)d.H * d.W, hw = (size_t)d.h * d.w;
    float acc[CPG];
#pragma unroll
    for (int c = 0; c < CPG; ++c) acc[c] = 0.f;
    for (int t = 0; t < d.T; ++t) {
        if (valid != nullptr && valid[b * d.T + t] == 0) continue;
        const float* ap = attn + ((size_t)(g * d.B + b) * d.T + t) * hw;
        const float a = ty.w0 * (tx.w0 * ap[ty.i0 * d.w + tx.i0] + tx.w1 * ap[ty.i0 * d.w + tx.i1]) +
                        ty.w1 * (tx.w0 * ap[ty.i1 * d.w + tx.i0] + tx.w1 * ap[ty.i1 * d.w + tx.i1]);
        const float* xp = x + (((size_t)b * d.T + t) * d.C + g * CPG) * HW + (size_t)Y * d.W + X;
#pragma unroll
        for (int c = 0; c < CPG; ++c) acc[c] += a * xp[(size_t)c * HW];
    }
    float* op = out + ((size_t)b * d.C + g * CPG) * HW + (size_t)Y * d.W + X;
#pragma unroll
    for (int c = 0; c < CPG; ++c) op[(size_t)c * HW] = acc[c];
}

// gx = up(attn) * gout ;  gup[g,b,t,Y,X] = sum_{c in g} x * gout.  GX = false: gup only, gx is neither read nor written.
// AUP (with GX = false): the interpolated weight goes to a_up[g,b,t,Y,X] instead of its products with gout to gx -- whoever
// adds to gx next forms round(a_up * gout) itself (c2s_conv4x4s2_dgrad_winograd_skip); of gx only the padded frames are
// written (zeros, unless gx_acc)
template <int CPG, bool GX = true, bool AUP = false>
__global__ __launch_bounds__(256) void agg_bwd_kernel(const float* __restrict__ x, const float* __restrict__ attn,
                                                      const int* __restrict__ valid, const float* __restrict__ gout,
                                                      float* __restrict__ gx, int gx_acc, float* __restrict__ gup,
                                                      float* __restrict__ a_up, c2s_agg_desc d) {
    const long total = (long)d.B * d.n_head * d.H * d.W;
    const long e = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int X = (int)(e % d.W);
    long r = e / d.W;
    const int Y = (int)(r % d.H); r /= d.H;
    const int g = (int)(r % d.n_head), b = (int)(r / d.n_head);
    const Taps ty = taps_for(Y, d.h, d.H), tx = taps_for(X, d.w, d.W);
    const size_t HW = (size_t)d.H * d.W, hw = (size_t)d.h * d.w;
    float go[CPG];
    const float* gp = gout + ((size_t)b * d.C + g * CPG) * HW + (size_t)Y * d.W + X;
#pragma unroll
    for (int c = 0; c < CPG; ++c) go[c] = gp[(size_t)c * HW];
    for (int t = 0; t < d.T; ++t) {
        const size_t xo = (((size_t)b * d.T + t) * d.C + g * CPG) * HW + (size_t)Y * d.W + X;
        const size_t uo = ((size_t)(g * d.B + b) * d.T + t) * HW + (size_t)Y * d.W + X;
        if (valid != nullptr && valid[b * d.T + t] == 0) {
            if ((GX || AUP) && !gx_acc) {
#pragma unroll
                for (int c = 0; c < CPG; ++c) gx[xo + (size_t)c * HW] = 0.f;
            }
            gup[uo] = 0.f;
            continue;
        }
        const float* ap = attn + ((size_t)(g * d.B + b) * d.T + t) * hw;
        const float a = ty.w0 * (tx.w0 * ap[ty.i0 * d.w + tx.i0] + tx.w1 * ap[ty.i0 * d.w + tx.i1]) +
                        ty.w1 * (tx.w0 * ap[ty.i1 * d.w + tx.i0] + tx.w1 * ap[ty.i1 * d.w + tx.i1]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CPG; ++c) {
            if constexpr (GX) {
                s += x[xo + (size_t)c * HW] * go[c];
                const float v = a * go[c];
                if (gx_acc) gx[xo + (size_t)c * HW] += v; else gx[xo + (size_t)c * HW] = v;
            } else {
                s = fmaf(x[xo + (size_t)c * HW], go[c], s);     // the contraction the form with gx compiles to
            }
        }
        gup[uo] = s;
        if constexpr (AUP) a_up[uo] = a;
    }
}

// Adjoint of the bilinear upsampling of the attention masks: gattn[plane][i][j] += sum_{Y,X} wy(Y,i) wx(X,j) gup[plane][Y][X].
// One workgroup per plane, separable, gup read once: thread X walks the rows Y = 0..H-1 of column X (coalesced row reads,
// AGG_ADJ_ROWS loads in flight) and keeps the running sums of the two low-resolution rows that row Y touches (i0 and
// i0 + 1; i0 never decreases with Y); a low-resolution row that Y has left is parked in LDS ([ni][cw + 1] floats, 8 KB at
// 16 x 128).  Then thread (i, j) folds the <= 3*W/w contributing columns of row i out of LDS.
// A plane whose parked rows would not fit AGG_ADJ_LDS_FLOATS is cut into tiles of nj low-resolution columns and ni rows;
// a tile reads one low-resolution cell of halo on each side (blockIdx.x = (plane * tiles_i + ti) * tiles_j + tj).
// Order of every sum: ascending Y, then ascending X, whatever the tiling, B, T or the grid.  The rows of weight exactly 0
// that a walk over [(i-1) H/h, (i+2) H/h) would also visit are left out: fma(0, v, acc) == acc for finite v, acc from +0.
constexpr int AGG_ADJ_ROWS = 8;
constexpr int AGG_ADJ_LDS_FLOATS = 8192;
constexpr int AGG_ADJ_MAX_LDS_FLOATS = 16384;

__global__ __launch_bounds__(256) void agg_upsample_adjoint_kernel(const float* __restrict__ gup, float* __restrict__ gattn,
                                                                   c2s_agg_desc d, int ni, int nj) {
    extern __shared__ float parked[];               // [ni][cw + 1]
    const int tiles_j = (d.w + nj - 1) / nj, tiles_i = (d.h + ni - 1) / ni;
    const int tj = blockIdx.x % tiles_j, ti = (blockIdx.x / tiles_j) % tiles_i;
    const long plane = blockIdx.x / (tiles_j * tiles_i);
    const int sy = d.H / d.h, sx = d.W / d.w;
    const int ia = ti * ni, ib = min(d.h, ia + ni), ja = tj * nj, jb = min(d.w, ja + nj);
    const int ya = max(0, (ia - 1) * sy), yb = min(d.H, (ib + 1) * sy);
    const int xa = max(0, (ja - 1) * sx), xb = min(d.W, (jb + 1) * sx);
    const int ld = xb - xa + 1;                     // + 1: lanes of neighbouring i fold out of different banks
    const float* gp = gup + (size_t)plane * d.H * d.W;
    for (int X = xa + threadIdx.x; X < xb; X += blockDim.x) {
        float* col = parked + (X - xa);
        int cur = taps_for(ya, d.h, d.H).i0;        // accA belongs to low-resolution row cur, accB to cur + 1
        float accA = 0.f, accB = 0.f;
        for (int i = ia; i < min(cur, ib); ++i) col[(i - ia) * ld] = 0.f;
        auto add_row = [&](int Y, float v) {
            const Taps ty = taps_for(Y, d.h, d.H);
            while (cur < ty.i0) {
                if (cur >= ia && cur < ib) col[(cur - ia) * ld] = accA;
                accA = accB; accB = 0.f; ++cur;
            }
            // the weights (ty.i0 == i ? ty.w0 : 0.f) + (ty.i1 == i ? ty.w1 : 0.f) at i = i0 and at i = i0 + 1
            const bool one = ty.i1 == ty.i0;
            accA = fmaf(ty.w0 + (one ? ty.w1 : 0.f), v, accA);
            if (!one) accB = fmaf(0.f + ty.w1, v, accB);
        };
        int Y = ya;
        for (; Y + AGG_ADJ_ROWS <= yb; Y += AGG_ADJ_ROWS) {
            float v[AGG_ADJ_ROWS];
#pragma unroll
            for (int k = 0; k < AGG_ADJ_ROWS; ++k) v[k] = gp[(size_t)(Y + k) * d.W + X];
#pragma unroll
            for (int k = 0; k < AGG_ADJ_ROWS; ++k) add_row(Y + k, v[k]);
        }
        for (; Y < yb; ++Y) add_row(Y, gp[(size_t)Y * d.W + X]);
        for (; cur < ib; ++cur) {
            if (cur >= ia) col[(cur - ia) * ld] = accA;
            accA = accB; accB = 0.f;
        }
    }
    __syncthreads();
    const int tw = jb - ja;
    for (int e = threadIdx.x; e < (ib - ia) * tw; e += blockDim.x) {
        const int i = ia + e / tw, j = ja + e % tw;
        const float* row = parked + (i - ia) * ld - xa;
        const int x0 = max(0, (j - 1) * sx), x1 = min(d.W, (j + 2) * sx);
        float acc = 0.f;
        for (int X = x0; X < x1; ++X) {
            const Taps tx = taps_for(X, d.w, d.W);
            const float wx = (tx.i0 == j ? tx.w0 : 0.f) + (tx.i1 == j ? tx.w1 : 0.f);
            acc = fmaf(wx, row[X], acc);
        }
        gattn[((size_t)plane * d.h + i) * d.w + j] += acc;
    }
}

// tile of the adjoint: the whole plane where its parked rows fit, else fewer low-resolution columns, then fewer rows
struct AdjointTile {
    int ni, nj, cw;                                 // low-resolution rows and columns of a tile; columns of gup it reads
};
AdjointTile adjoint_tile(const c2s_agg_desc* d) {
    const int sx = d->W / d->w;
    auto cw = [&](int n) { return n >= d->w || (n + 2) * sx > d->W ? d->W : (n + 2) * sx; };
    auto fits = [&](int n_i, int n_j) { return (long)n_i * (cw(n_j) + 1) <= AGG_ADJ_LDS_FLOATS; };
    int ni = d->h, nj = d->w;
    while (nj > 1 && !fits(ni, nj) && cw(nj) > 1024) nj = (nj + 1) / 2;
    while (ni > 1 && !fits(ni, nj)) ni = (ni + 1) / 2;
    while (nj > 1 && !fits(ni, nj)) nj = (nj + 1) / 2;
    return {ni, nj, cw(nj)};
}

// ---- agg_mode "att_mean" / "mean" (temporal_aggregator.py:46-56,71-77) reuse the kernels above with a derived weight tensor:
//   att_mean: every channel group gets the head-averaged attention  v[g] = mean_h attn[h]   (g = 0..n_head-1)
//   mean    : v[g][b][t] = valid[b,t] / #valid frames of b          (one weight per frame: a 1x1 "attention map")
__global__ __launch_bounds__(256) void head_mean_kernel(const float* __restrict__ attn, float* __restrict__ v, int n_head, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int h = 0; h < n_head; ++h) s += attn[(size_t)h * n + i];
    s /= (float)n_head;
    for (int h = 0; h < n_head; ++h) v[(size_t)h * n + i] = s;
}
__global__ __launch_bounds__(256) void head_mean_bwd_kernel(const float* __restrict__ gv, float* __restrict__ gattn, int n_head,
                                                            long n, int accumulate) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int h = 0; h < n_head; ++h) s += gv[(size_t)h * n + i];
    s /= (float)n_head;
    for (int h = 0; h < n_head; ++h) gattn[(size_t)h * n + i] = accumulate ? gattn[(size_t)h * n + i] + s : s;
}
__global__ void frame_mean_weights_kernel(const int* __restrict__ valid, float* __restrict__ v, int n_head, int B, int T) {
    const int b = blockIdx.x;
    int cnt = 0;
    for (int t = 0; t < T; ++t) cnt += (valid == nullptr || valid[b * T + t] != 0) ? 1 : 0;
    const float w = 1.f / (float)cnt;
    for (int e = threadIdx.x; e < n_head * T; e += blockDim.x) {
        const int h = e / T, t = e % T;
        v[((size_t)h * B + b) * T + t] = (valid == nullptr || valid[b * T + t] != 0) ? w : 0.f;
    }
}

int check(const c2s_agg_desc* d) {
    C2S_REQUIRE(d && d->B > 0 && d->T > 0 && d->C > 0 && d->H > 0 && d->W > 0, "aggregate: bad shape");
    C2S_REQUIRE(d->n_head > 0 && d->C % d->n_head == 0, "aggregate: C %% n_head != 0");
    C2S_REQUIRE(d->H >= d->h && d->W >= d->w && d->H % d->h == 0 && d->W % d->w == 0,
                "aggregate: feature maps must be an integer multiple of the attention resolution");
    const int cpg = d->C / d->n_head;
    C2S_REQUIRE(cpg == 1 || cpg == 2 || cpg == 4 || cpg == 8 || cpg == 16, "aggregate: C/n_head must be 1,2,4,8 or 16");
    return C2S_OK;
}

}  // namespace

extern "C" int c2s_attn_head_mean(const float* attn, float* v, int n_head, long n, void* stream) {
    C2S_REQUIRE(attn && v && n_head > 0 && n > 0, "attn_head_mean: bad args");
    C2S_REQUIRE_ITEMS(n, 256, "attn_head_mean");
    hipLaunchKernelGGL(head_mean_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, attn, v, n_head, n);
    C2S_CHECK_LAUNCH("attn_head_mean");
    return C2S_OK;
}
extern "C" int c2s_attn_head_mean_bwd(const float* gv, float* gattn, int n_head, long n, int accumulate, void* stream) {
    C2S_REQUIRE(gv && gattn && n_head > 0 && n > 0, "attn_head_mean_bwd: bad args");
    C2S_REQUIRE_ITEMS(n, 256, "attn_head_mean_bwd");
    hipLaunchKernelGGL(head_mean_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, gv, gattn, n_head, n, accumulate);
    C2S_CHECK_LAUNCH("attn_head_mean_bwd");
    return C2S_OK;
}
extern "C" int c2s_frame_mean_weights(const int* valid, float* v, int n_head, int B, int T, void* stream) {
    C2S_REQUIRE(v && n_head > 0 && B > 0 && T > 0, "frame_mean_weights: bad args");
    hipLaunchKernelGGL(frame_mean_weights_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, valid, v, n_head, B, T);
    C2S_CHECK_LAUNCH("frame_mean_weights");
    return C2S_OK;
}

extern "C" int c2s_temporal_aggregate_fwd(const c2s_agg_desc* d, const float* x, const float* attn, const int* valid,
                                          float* out, void* stream) {
    if (int rc = check(d)) return rc;
    C2S_REQUIRE(x && attn && out, "aggregate_fwd: null pointer");
    const long total = (long)d->B * d->n_head * d->H * d->W;
    C2S_REQUIRE_ITEMS(total, 256, "aggregate_fwd");
    dim3 grid(cdiv(total, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (d->C / d->n_head) {
        case 1: hipLaunchKernelGGL(agg_fwd_kernel<1>, grid, block, 0, st, x, attn, valid, out, *d); break;
        case 2: hipLaunchKernelGGL(agg_fwd_kernel<2>, grid, block, 0, st, x, attn, valid, out, *d); break;
        case 4: hipLaunchKernelGGL(agg_fwd_kernel<4>, grid, block, 0, st, x, attn, valid, out, *d); break;
        case 8: hipLaunchKernelGGL(agg_fwd_kernel<8>, grid, block, 0, st, x, attn, valid, out, *d); break;
        default: hipLaunchKernelGGL(agg_fwd_kernel<16>, grid, block, 0, st, x, attn, valid, out, *d); break;
    }
    C2S_CHECK_LAUNCH("aggregate_fwd");
    return C2S_OK;
}

extern "C" size_t c2s_temporal_aggregate_bwd_workspace_floats(const c2s_agg_desc* d) {
    if (!d) return 0;
    return (size_t)d->n_head * d->B * d->T * d->H * d->W;
}

namespace {

// a_up == NULL: gx = up(attn) * gout (or nothing where gx == NULL); a_up != NULL: the weight itself goes to a_up
int aggregate_bwd(const c2s_agg_desc* d, const float* x, const float* attn, const int* valid, const float* gout, float* gx,
                  int gx_accumulate, float* gattn, float* a_up, float* workspace, size_t ws_floats, void* stream) {
    if (int rc = check(d)) return rc;
    // gx == NULL: only gattn (the input needs no gradient); gattn == NULL: only gx (the attention masks need none)
    C2S_REQUIRE(x && attn && gout && (gx || gattn) && workspace, "aggregate_bwd: null pointer");
    C2S_REQUIRE(ws_floats >= c2s_temporal_aggregate_bwd_workspace_floats(d), "aggregate_bwd: workspace too small");
    const AdjointTile tile = adjoint_tile(d);
    const long lds_floats = (long)tile.ni * (tile.cw + 1);
    const long tiles = (long)d->n_head * d->B * d->T * cdiv(d->h, tile.ni) * cdiv(d->w, tile.nj);
    if (gattn != nullptr) {
        C2S_REQUIRE(lds_floats <= AGG_ADJ_MAX_LDS_FLOATS, "aggregate_bwd: W / w too large for the upsample adjoint");
        C2S_REQUIRE(tiles <= 0x7fffffffL, "aggregate_bwd: too many planes for the upsample adjoint");
    }
    const long total = (long)d->B * d->n_head * d->H * d->W;
    C2S_REQUIRE_ITEMS(total, 256, "aggregate_bwd");
    dim3 grid(cdiv(total, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
#define C2S_AGG_BWD(CPG_)                                                                                                    \
    if (a_up != nullptr) hipLaunchKernelGGL((agg_bwd_kernel<CPG_, false, true>), grid, block, 0, st, x, attn, valid, gout, gx, gx_accumulate, workspace, a_up, *d); \
    else if (gx != nullptr) hipLaunchKernelGGL(agg_bwd_kernel<CPG_>, grid, block, 0, st, x, attn, valid, gout, gx, gx_accumulate, workspace, a_up, *d); \
    else hipLaunchKernelGGL((agg_bwd_kernel<CPG_, false>), grid, block, 0, st, x, attn, valid, gout, gx, 0, workspace, a_up, *d);
    switch (d->C / d->n_head) {
        case 1: C2S_AGG_BWD(1) break;
        case 2: C2S_AGG_BWD(2) break;
        case 4: C2S_AGG_BWD(4) break;
        case 8: C2S_AGG_BWD(8) break;
        default: C2S_AGG_BWD(16) break;
    }
#undef C2S_AGG_BWD
    C2S_CHECK_LAUNCH("aggregate_bwd");
    if (gattn == nullptr) return C2S_OK;
    const int threads = tile.cw >= 256 ? 256 : (tile.cw > 64 ? 128 : 64);
    hipLaunchKernelGGL(agg_upsample_adjoint_kernel, dim3(tiles), dim3(threads), (size_t)lds_floats * sizeof(float), st,
                       workspace, gattn, *d, tile.ni, tile.nj);
    C2S_CHECK_LAUNCH("aggregate_upsample_adjoint");
    return C2S_OK;
}

// gx[b,t,c] = round(a_up[g,b,t] * gskip[b,c]) on the real frames: the product agg_bwd_kernel<CPG, true> stores
__global__ __launch_bounds__(256) void agg_skip_term_kernel(const float* __restrict__ a_up, const float* __restrict__ gskip,
                                                            const int* __restrict__ valid, float* __restrict__ gx,
                                                            c2s_agg_desc d) {
    const size_t HW = (size_t)d.H * d.W;
    const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (e >= (size_t)d.B * d.T * d.C * HW) return;
    const size_t pix = e % HW;
    size_t r = e / HW;
    const int c = (int)(r % d.C); r /= d.C;
    const int t = (int)(r % d.T), b = (int)(r / d.T);
    if (valid != nullptr && valid[b * d.T + t] == 0) return;
    const int g = c / (d.C / d.n_head);
    gx[e] = a_up[((size_t)(g * d.B + b) * d.T + t) * HW + pix] * gskip[((size_t)b * d.C + c) * HW + pix];
}

}  // namespace

extern "C" int c2s_temporal_aggregate_bwd(const c2s_agg_desc* d, const float* x, const float* attn, const int* valid,
                                          const float* gout, float* gx, int gx_accumulate, float* gattn,
                                          float* workspace, size_t ws_floats, void* stream) {
    return aggregate_bwd(d, x, attn, valid, gout, gx, gx_accumulate, gattn, nullptr, workspace, ws_floats, stream);
}

extern "C" int c2s_temporal_aggregate_bwd_skip(const c2s_agg_desc* d, const float* x, const float* attn, const int* valid,
                                               const float* gout, float* gx, int gx_accumulate, float* gattn, float* a_up,
                                               float* workspace, size_t ws_floats, void* stream) {
    C2S_REQUIRE(gx && gattn && a_up, "aggregate_bwd_skip: null pointer");
    return aggregate_bwd(d, x, attn, valid, gout, gx, gx_accumulate, gattn, a_up, workspace, ws_floats, stream);
}

extern "C" int c2s_agg_skip_term(const c2s_agg_desc* d, const float* a_up, const float* gskip, const int* valid, float* gx,
                                 void* stream) {
    if (int rc = check(d)) return rc;
    C2S_REQUIRE(a_up && gskip && gx, "agg_skip_term: null pointer");
    const size_t n = (size_t)d->B * d->T * d->C * d->H * d->W;
    C2S_REQUIRE_ITEMS(n, 256, "agg_skip_term");       // one thread per element of x
    hipLaunchKernelGGL(agg_skip_term_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a_up, gskip,
                       valid, gx, *d);
    C2S_CHECK_LAUNCH("agg_skip_term");
    return C2S_OK;
}
