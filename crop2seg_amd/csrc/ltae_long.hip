// Time-chunked L-TAE family: the same function as the families of ltae.hip (see the header of that file for the
// re-association), for series of any length.  Those families hold a whole series per workgroup (registers, LDS tiles of
// [T][16][pixels], or a float[64] per lane) and stop at T = 64; here nothing is held per time step: the time axis is walked
// in chunks, and what has to survive a sweep over T lives in HBM (attn_pre as the raw-score scratch, GS) or is a running
// quantity per lane (softmax max / sum, dot products, z, V, Z).
//
// Layout: 64-pixel tiles, lane = pixel: every global access is one 256-byte row segment.  A workgroup is 16 waves on one
// tile.  In the per-head kernels wave = head, so U[h][c] and Wc[16h+j][c] are wave-uniform (scalar cache); x comes in
// chunks of 256 rows [t][c] of the tile, staged in LDS (normalised on the way) while the next chunk is in flight.
//
//   forward  F1 statistics   wave = GroupNorm group: exact two-pass moments per chunk of 32 values, Chan merges across chunks
//            F2 attention    wave = head:  sweep 1  scores (x chunks), running max / sum, raw scores -> attn_pre
//                                          sweep 2  softmax, dropout, attn / attn_pre, sum_t a, sum_t a pe -> emb
//                                          sweep 3  z[h][c] = sum_t a xhat_t (x chunks, 32 channels per pass), emb += Wc z
//   backward B1 heads        wave = head:  sweep A  dot x: r[h][c] xhat_t (32 channels per pass, partial sums in GS)
//                                          sweep B  ga = (dot x + ge.(bc + pe_t) + g_attn) keep -> GS, dot = sum_t a' ga
//                                          sweep C  gs = a' (ga - dot) -> GS; d s0, d bc partials; sum_t a, sum_t gs
//            B2 V, Z         wave = head:  Zn = sum_t a xn, Vn = sum_t gs xn (16 channels per pass) -> Z, d U partials;
//                                          head sums of the GroupNorm backward through LDS: d gamma, d beta partials and
//                                          the means m1, m2 in closed form (no extra pass over T)
//            B3 dx           wave = 4 channels: attn / gs chunks of 16 steps in LDS; gx = rstd (gamma dxhat - m1 - xn m2)
// x is read three times per direction.  Every partial is written per tile and summed by the fixed-order reductions of
// ltae.hip: gradients are bitwise reproducible run to run.
#include "ltae_drop.h"
#include "ltae_long.h"

namespace {

constexpr int NH = 16, DV = 16, DM = NH * DV;
constexpr int XROWS = 256;                       // rows [t][c] of one staged x chunk

struct LongTile {
    int b, pix0, pix, lane;
    bool act;
    long pidx;
};
__device__ __forceinline__ LongTile long_tile(int HW) {
    LongTile t;
    const int tpb = (HW + LONG_PX - 1) / LONG_PX;
    t.lane = threadIdx.x & 63;
    t.b = blockIdx.x / tpb;
    t.pix0 = (blockIdx.x % tpb) * LONG_PX;
    t.act = t.pix0 + t.lane < HW;
    t.pix = t.act ? t.pix0 + t.lane : HW - 1;        // inactive lanes read a valid pixel and write nothing
    t.pidx = (long)t.b * HW + t.pix;
    return t;
}
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// x chunk of NCB channels [cb, cb + NCB) x (256 / NCB) time steps from t0: wave w loads rows w, w + 16, ...  (16 per lane,
// all in flight); rows beyond T are 0
template <int NCB>
__device__ __forceinline__ void load_rows(float (&nx)[16], const LtaeLongArgs& a, const LongTile& tl, int t0, int cb) {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = w + 16 * k, tt = i / NCB, c = cb + i % NCB, t = t0 + tt;
        nx[k] = t < a.T ? a.x[(((size_t)tl.b * a.T + t) * a.C + c) * a.HW + tl.pix] : 0.f;
    }
}
// -> LDS xs[i][lane], normalised: xn = (x - mean) rstd, AFFINE: xhat = gamma xn + beta.  STl [16][2][64] = mean, rstd.
template <int NCB, bool AFFINE>
__device__ __forceinline__ void put_rows(float* xs, const float (&nx)[16], const LtaeLongArgs& a, const float* STl, int cb,
                                         int cpg) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = w + 16 * k, c = cb + i % NCB, g = c / cpg;
        float v = (nx[k] - STl[g * 128 + lane]) * STl[g * 128 + 64 + lane];
        if (AFFINE) v = fmaf(v, a.gamma[c], a.beta[c]);
        xs[i * 64 + lane] = v;
    }
}

__device__ __forceinline__ float keep_of(const LtaeLongArgs& a, const DropCtx& dc, long row, int t, uint32_t& bits) {
    if (a.drop_p <= 0.f) return 1.f;
    if (a.keep != nullptr) return a.keep[(size_t)row * a.T + t] != 0.f ? 1.f / (1.f - a.drop_p) : 0.f;
    if ((t & 1) == 0) bits = drop_bits(dc, row, t >> 1);
    return drop_pick(dc, bits, t);
}

// ------------------------------------------------------------------------------------------ F1 statistics
// GroupNorm over (C/16 x T) per (pixel, group), padded frames included (tae.py:461).  Chunks of TS steps x CPG channels
// (32 values): exact two-pass moments of the chunk, Chan merge into the running (mean, M2).
template <int CPG>
__global__ __launch_bounds__(1024) void ltae_long_stats_kernel(LtaeLongArgs a) {
    const LongTile tl = long_tile(a.HW);
    const int g = wave_id(), T = a.T;
    constexpr int TS = 32 / CPG;
    const float* xp = a.x + ((size_t)tl.b * T * a.C + (size_t)g * CPG) * a.HW + tl.pix;
    float mean = 0.f, m2 = 0.f, cnt = 0.f;
    for (int t0 = 0; t0 < T; t0 += TS) {
        const int nt = T - t0 < TS ? T - t0 : TS;
        float v[TS * CPG];
#pragma unroll
        for (int i = 0; i < TS * CPG; ++i)
            v[i] = i / CPG < nt ? xp[((size_t)(t0 + i / CPG) * a.C + i % CPG) * a.HW] : 0.f;
        float sb = 0.f;
#pragma unroll
        for (int i = 0; i < TS * CPG; ++i) sb += v[i];          // zeros beyond T add nothing
        const float nb = (float)(nt * CPG), mb = sb / nb;
        float qb = 0.f;
#pragma unroll
        for (int i = 0; i < TS * CPG; ++i)
            if (i / CPG < nt) {
                const float d = v[i] - mb;
                qb = fmaf(d, d, qb);
            }
        const float tot = cnt + nb, delta = mb - mean;
        mean = fmaf(delta, nb / tot, mean);
        m2 += qb + delta * delta * (cnt * nb / tot);
        cnt = tot;
    }
    const float rstd = rsqrtf(fmaxf(m2 / cnt, 0.f) + a.eps);
    if (tl.act) {
        a.stats[(tl.pidx * NH + g) * 2] = mean;
        a.stats[(tl.pidx * NH + g) * 2 + 1] = rstd;
    }
}

// ------------------------------------------------------------------------------------------ F2 attention, emb
constexpr size_t HEADS_LDS = (size_t)(XROWS * 64 + NH * 128) * sizeof(float);

template <int C>
__global__ __launch_bounds__(1024) void ltae_long_fwd_kernel(LtaeLongArgs a) {
    extern __shared__ float lds[];
    float* xs = lds;                    // [256 rows][64 px]
    float* STl = xs + XROWS * 64;       // [16 groups][mean, rstd][64 px]
    constexpr int cpg = C / NH;
    const LongTile tl = long_tile(a.HW);
    const int h = wave_id(), lane = tl.lane, T = a.T, HW = a.HW, b = tl.b;
    STl[h * 128 + lane] = a.stats[(tl.pidx * NH + h) * 2];
    STl[h * 128 + 64 + lane] = a.stats[(tl.pidx * NH + h) * 2 + 1];
    const size_t orow = (size_t)(h * a.B + b) * T * HW + tl.pix;       // attn [16,B,T,HW] of (h, b, pixel): + t*HW
    const float* Uh = a.U + h * C;

    // sweep 1: scores of 256 / C steps per chunk; running max / sum; raw (masked) scores -> attn_pre
    constexpr int TC1 = XROWS / C;
    float nx[16];
    load_rows<C>(nx, a, tl, 0, 0);
    float mx = -3.0e38f, den = 0.f, den_lo = 0.f;      // compensated running sum: T reaches the hundreds
    for (int t0 = 0; t0 < T; t0 += TC1) {
        __syncthreads();
        put_rows<C, true>(xs, nx, a, STl, 0, cpg);
        __syncthreads();
        if (t0 + TC1 < T) load_rows<C>(nx, a, tl, t0 + TC1, 0);
        for (int tt = 0; tt < TC1 && t0 + tt < T; ++tt) {
            const int t = t0 + tt;
            const float* xr = xs + tt * C * 64 + lane;
            float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 16
            for (int c = 0; c < C; ++c) s4[c & 3] = fmaf(Uh[c], xr[c * 64], s4[c & 3]);
            float s = a.s0[((size_t)b * T + t) * NH + h] + ((s4[0] + s4[1]) + (s4[2] + s4[3]));
            if (a.valid != nullptr && a.valid[b * T + t] == 0) s = -1e6f;         // tae.py:831
            const float nm = fmaxf(mx, s), f = __expf(mx - nm);
            den *= f;
            den_lo *= f;
            const float y = __expf(s - nm) - den_lo, sum = den + y;
            den_lo = (sum - den) - y;
            den = sum;
            mx = nm;
            if (tl.act) a.attn_pre[orow + (size_t)t * HW] = s;
        }
    }
    __syncthreads();        // the wave's score stores are complete before sweep 2 reads them back

    // sweep 2: softmax, dropout; sum_t a and sum_t a pe_t (pe through the scalar cache) start the embedding
    const float inv = 1.f / den;
    const long Ptot = (long)a.B * HW, row = (long)h * Ptot + tl.pidx;
    DropCtx dc = {};
    if (a.drop_p > 0.f && a.keep == nullptr) dc = drop_ctx_of(a.seed, a.seed_dev, a.drop_p, T);
    uint32_t bits = 0;
    float asum = 0.f, ape[DV];
#pragma unroll
    for (int j = 0; j < DV; ++j) ape[j] = 0.f;
    for (int t = 0; t < T; ++t) {
        const size_t o = orow + (size_t)t * HW;
        const float av = __expf(a.attn_pre[o] - mx) * inv;
        const float ad = av * keep_of(a, dc, row, t, bits);
        if (tl.act) {
            a.attn_pre[o] = av;
            a.attn[o] = ad;
        }
        asum += ad;
        if (a.emb != nullptr) {
            const float* pt = a.pe + ((size_t)b * T + t) * DV;
#pragma unroll
            for (int j = 0; j < DV; ++j) ape[j] = fmaf(ad, pt[j], ape[j]);
        }
    }
    if (a.emb == nullptr) return;   // W-TAE: attention masks only (tae.py:619)
    float* embp = a.emb + ((size_t)b * DM + h * DV) * HW + tl.pix;
    if (tl.act) {
#pragma unroll
        for (int j = 0; j < DV; ++j) embp[(size_t)j * HW] = fmaf(asum, a.bc[h * DV + j], ape[j]);
    }

    // sweep 3: z[c] = sum_t a_t xhat_t[c] for 32 channels per pass (x chunks of 8 steps), then emb += Wc_h z
    float e[DV];
#pragma unroll
    for (int j = 0; j < DV; ++j) e[j] = 0.f;
    for (int cb = 0; cb < C; cb += 32) {
        float z[32];
#pragma unroll
        for (int c = 0; c < 32; ++c) z[c] = 0.f;
        load_rows<32>(nx, a, tl, 0, cb);
        for (int t0 = 0; t0 < T; t0 += 8) {
            float ad8[8];
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) ad8[tt] = t0 + tt < T ? a.attn[orow + (size_t)(t0 + tt) * HW] : 0.f;
            __syncthreads();
            put_rows<32, true>(xs, nx, a, STl, cb, cpg);
            __syncthreads();
            if (t0 + 8 < T) load_rows<32>(nx, a, tl, t0 + 8, cb);
#pragma unroll
            for (int c = 0; c < 32; ++c) {          // per-chunk partial first: the rounding grows with 8 + T / 8, not T
                float zc = 0.f;
#pragma unroll
                for (int tt = 0; tt < 8; ++tt) zc = fmaf(ad8[tt], xs[(tt * 32 + c) * 64 + lane], zc);      // rows beyond T are 0
                z[c] += zc;
            }
        }
#pragma unroll
        for (int j = 0; j < DV; ++j) {
            const float* wr = a.Wc + (size_t)(h * DV + j) * C + cb;
#pragma unroll
            for (int c = 0; c < 32; ++c) e[j] = fmaf(wr[c], z[c], e[j]);
        }
    }
    if (tl.act) {
#pragma unroll
        for (int j = 0; j < DV; ++j) embp[(size_t)j * HW] += e[j];
    }
}

// ------------------------------------------------------------------------------------------ B1 heads
template <int C>
__global__ __launch_bounds__(1024) void ltae_long_bwd_heads_kernel(LtaeLongArgs a) {
    extern __shared__ float lds[];
    float* xs = lds;
    float* STl = xs + XROWS * 64;
    constexpr int cpg = C / NH;
    const LongTile tl = long_tile(a.HW);
    const int h = wave_id(), lane = tl.lane, T = a.T, HW = a.HW, b = tl.b;
    STl[h * 128 + lane] = a.stats_in[(tl.pidx * NH + h) * 2];
    STl[h * 128 + 64 + lane] = a.stats_in[(tl.pidx * NH + h) * 2 + 1];
    const size_t orow = (size_t)(h * a.B + b) * T * HW + tl.pix;
    float ge[DV];
#pragma unroll
    for (int j = 0; j < DV; ++j) ge[j] = a.g_emb != nullptr ? a.g_emb[((size_t)b * DM + h * DV + j) * HW + tl.pix] : 0.f;

    // sweep A: GS[h,t] = sum_c r[h][c] xhat_t[c], r = Wc_h^T ge_h, 32 channels per pass (the later passes add to GS)
    if (a.g_emb != nullptr) {
        float nx[16];
        for (int cb = 0; cb < C; cb += 32) {
            float r[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) r[c] = 0.f;
#pragma unroll
            for (int j = 0; j < DV; ++j) {
                const float* wr = a.Wc + (size_t)(h * DV + j) * C + cb;
#pragma unroll
                for (int c = 0; c < 32; ++c) r[c] = fmaf(ge[j], wr[c], r[c]);
            }
            load_rows<32>(nx, a, tl, 0, cb);
            for (int t0 = 0; t0 < T; t0 += 8) {
                __syncthreads();
                put_rows<32, true>(xs, nx, a, STl, cb, cpg);
                __syncthreads();
                if (t0 + 8 < T) load_rows<32>(nx, a, tl, t0 + 8, cb);
                for (int tt = 0; tt < 8 && t0 + tt < T; ++tt) {
                    const float* xr = xs + tt * 32 * 64 + lane;
                    float d4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < 32; ++c) d4[c & 3] = fmaf(r[c], xr[c * 64], d4[c & 3]);
                    const float d = (d4[0] + d4[1]) + (d4[2] + d4[3]);
                    const size_t o = orow + (size_t)(t0 + tt) * HW;
                    if (tl.act) a.GS[o] = cb == 0 ? d : a.GS[o] + d;
                }
            }
        }
        __syncthreads();
    }

    // sweep B: ga = (dot x + ge.(bc + pe_t) + g_attn) * keep -> GS;  dot = sum_t a' ga
    float gebc = 0.f;
#pragma unroll
    for (int j = 0; j < DV; ++j) gebc = fmaf(ge[j], a.bc[h * DV + j], gebc);
    const long Ptot = (long)a.B * HW, row = (long)h * Ptot + tl.pidx;
    DropCtx dc = {};
    if (a.drop_p > 0.f && a.keep == nullptr) dc = drop_ctx_of(a.seed, a.seed_dev, a.drop_p, T);
    uint32_t bits = 0;
    float dot = 0.f, dot_lo = 0.f, asum = 0.f;
    for (int t = 0; t < T; ++t) {
        const size_t o = orow + (size_t)t * HW;
        float ga = gebc;
        if (a.g_emb != nullptr) {
            ga += a.GS[o];
            const float* pt = a.pe + ((size_t)b * T + t) * DV;
#pragma unroll
            for (int j = 0; j < DV; ++j) ga = fmaf(ge[j], pt[j], ga);
        }
        if (a.g_attn != nullptr) ga += a.g_attn[o];
        ga *= keep_of(a, dc, row, t, bits);
        const float y = a.attn_pre_in[o] * ga - dot_lo, sum = dot + y;        // compensated, as the forward's sum
        dot_lo = (sum - dot) - y;
        dot = sum;
        asum += a.attn_in[o];
        if (tl.act) a.GS[o] = ga;
    }
    __syncthreads();

    // sweep C: gs = a' (ga - dot) -> GS; d s0[b,t,h] partial of the tile (sum over the 64 lanes, fixed order)
    float gssum = 0.f;
    for (int t = 0; t < T; ++t) {
        const size_t o = orow + (size_t)t * HW;
        const float gs = a.attn_pre_in[o] * (a.GS[o] - dot);
        if (tl.act) a.GS[o] = gs;
        gssum += gs;
        const float red = wave_sum(tl.act ? gs : 0.f);
        if (lane == 0) a.part_s0[((size_t)blockIdx.x * T + t) * NH + h] = red;
    }
#pragma unroll
    for (int j = 0; j < DV; ++j) {
        const float red = wave_sum(tl.act ? ge[j] * asum : 0.f);
        if (lane == 0) a.part_bc[(size_t)blockIdx.x * DM + h * DV + j] = red;
    }
    if (tl.act) {
        a.ASG[(size_t)h * Ptot + tl.pidx] = asum;
        a.ASG[(size_t)(NH + h) * Ptot + tl.pidx] = gssum;
    }
}

// ------------------------------------------------------------------------------------------ B2 V, Z, GroupNorm-backward means
// Per (pixel, head), 16 channels per pass: Zn = sum_t attn xn, Vn = sum_t gs xn (xn = (x - mean) rstd).  Then
//   Z = gamma Zn + beta sum_t attn (-> d Wc),  V = gamma Vn + beta sum_t gs (-> d U partial),
//   q0[c] = sum_t dxhat[t][c]      = sum_h (sum_t attn) r[h][c] + (sum_t gs) U[h][c]    -> d beta,  m1 = mean_g gamma q0
//   q1[c] = sum_t dxhat[t][c] xn   = sum_h r[h][c] Zn[h][c] + U[h][c] Vn[h][c]          -> d gamma, m2 = mean_g gamma q1
// the head sums go through LDS, 16 channels at a time (thread = (channel, pixel) after the exchange).
constexpr size_t VZ_LDS = (size_t)(XROWS * 64 + NH * 128 + 16 * 64) * sizeof(float);

template <int C>
__global__ __launch_bounds__(1024) void ltae_long_bwd_vz_kernel(LtaeLongArgs a) {
    extern __shared__ float lds[];
    float* xs = lds;                    // x chunks [16 t][16 c][64 px]; then the head-sum exchange [16 h][16 c][64 px]
    float* STl = xs + XROWS * 64;
    float* GQ = STl + NH * 128;         // [16 c][64 px]  gamma q of the exchange's channels
    constexpr int cpg = C / NH;
    const LongTile tl = long_tile(a.HW);
    const int w = wave_id(), h = w, lane = tl.lane, T = a.T, HW = a.HW, b = tl.b;
    STl[w * 128 + lane] = a.stats_in[(tl.pidx * NH + w) * 2];
    STl[w * 128 + 64 + lane] = a.stats_in[(tl.pidx * NH + w) * 2 + 1];
    const size_t orow = (size_t)(h * a.B + b) * T * HW + tl.pix;
    const long Ptot = (long)a.B * HW;
    const float asum = a.ASG[(size_t)h * Ptot + tl.pidx], gssum = a.ASG[(size_t)(NH + h) * Ptot + tl.pidx];
    const float inv_n = 1.f / (float)(cpg * T);
    for (int cb = 0; cb < C; cb += 16) {
        float Zn[16], Vn[16], nx[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) Zn[c] = Vn[c] = 0.f;
        load_rows<16>(nx, a, tl, 0, cb);
        for (int t0 = 0; t0 < T; t0 += 16) {
            float ad[16], gs[16];
#pragma unroll
            for (int tt = 0; tt < 16; ++tt) {
                const bool in = t0 + tt < T;
                const size_t o = orow + (size_t)(in ? t0 + tt : 0) * HW;
                ad[tt] = in ? a.attn_in[o] : 0.f;
                gs[tt] = in ? a.GS[o] : 0.f;
            }
            __syncthreads();
            put_rows<16, false>(xs, nx, a, STl, cb, cpg);
            __syncthreads();
            if (t0 + 16 < T) load_rows<16>(nx, a, tl, t0 + 16, cb);
#pragma unroll
            for (int c = 0; c < 16; ++c) {          // per-chunk partials first, as in the forward's z
                float zc = 0.f, vc = 0.f;
#pragma unroll
                for (int tt = 0; tt < 16; ++tt) {
                    const float xv = xs[(tt * 16 + c) * 64 + lane];
                    zc = fmaf(ad[tt], xv, zc);
                    vc = fmaf(gs[tt], xv, vc);
                }
                Zn[c] += zc;
                Vn[c] += vc;
            }
        }
        // Z (for d Wc) and the d U partial of this head
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int cg = cb + c;
            const float gam = a.gamma[cg], bet = a.beta[cg];
            if (a.g_emb != nullptr && tl.act) a.Z[(((size_t)b * NH + h) * C + cg) * HW + tl.pix] = fmaf(gam, Zn[c], bet * asum);
            const float red = wave_sum(tl.act ? fmaf(gam, Vn[c], bet * gssum) : 0.f);
            if (lane == 0) a.part_U[((size_t)blockIdx.x * NH + h) * C + cg] = red;
        }
        float ge[DV];
#pragma unroll
        for (int j = 0; j < DV; ++j) ge[j] = a.g_emb != nullptr ? a.g_emb[((size_t)b * DM + h * DV + j) * HW + tl.pix] : 0.f;
        {
            constexpr int half = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {           // k = 0: q0 (d beta, m1), k = 1: q1 (d gamma, m2)
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const int cc = half * 16 + c, cg = cb + cc;
                    float r = 0.f;
#pragma unroll
                    for (int j = 0; j < DV; ++j) r = fmaf(ge[j], a.Wc[(size_t)(h * DV + j) * C + cg], r);
                    const float u = a.U[h * C + cg];
                    xs[(h * 16 + c) * 64 + lane] = k == 0 ? fmaf(asum, r, gssum * u) : fmaf(r, Zn[cc], u * Vn[cc]);
                }
                __syncthreads();
                {   // thread = (channel w of the 16, pixel): sum over the heads in order
                    const int cg = cb + half * 16 + w;
                    float q = 0.f;
#pragma unroll
                    for (int hh = 0; hh < NH; ++hh) q += xs[(hh * 16 + w) * 64 + lane];
                    const float red = wave_sum(tl.act ? q : 0.f);
                    if (lane == 0) a.part_gb[((size_t)blockIdx.x * C + cg) * 2 + (k == 1 ? 0 : 1)] = red;   // (d gamma, d beta)
                    GQ[w * 64 + lane] = a.gamma[cg] * q;
                }
                __syncthreads();
                if (w < 16 / cpg) {                  // the groups of these 16 channels (cpg divides 16)
                    const int g = (cb + half * 16) / cpg + w;
                    float m = 0.f;
                    for (int i = 0; i < cpg; ++i) m += GQ[(w * cpg + i) * 64 + lane];
                    if (tl.act) a.M[(tl.pidx * NH + g) * 2 + k] = m * inv_n;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ B3 dx
// gx[t][c] = rstd (gamma_c sum_h (attn[h,t] r[h][c] + gs[h,t] U[h][c]) - m1 - xn m2).  Wave = 4 channels (one group), 64
// channels per pass; attn and gs of 16 steps x 16 heads staged in LDS; r[16][4] in registers, U through the scalar cache.
constexpr int GX_TC = 16;
constexpr size_t GX_LDS = (size_t)2 * GX_TC * NH * 64 * sizeof(float);

__global__ __launch_bounds__(1024) void ltae_long_bwd_gx_kernel(LtaeLongArgs a) {
    extern __shared__ float lds[];
    float* AGl = lds;                        // [16 t][16 h][64 px] attn
    float* GGl = AGl + GX_TC * NH * 64;      // [16 t][16 h][64 px] gs
    const LongTile tl = long_tile(a.HW);
    const int w = wave_id(), lane = tl.lane, T = a.T, HW = a.HW, C = a.C, b = tl.b, cpg = C / NH;
    for (int cb = 0; cb < C; cb += 64) {
        const int c4 = cb + 4 * w, g = c4 / cpg;
        const float mean = a.stats_in[(tl.pidx * NH + g) * 2], rstd = a.stats_in[(tl.pidx * NH + g) * 2 + 1];
        const float m1 = a.M[(tl.pidx * NH + g) * 2], m2 = a.M[(tl.pidx * NH + g) * 2 + 1];
        float r[NH][4];
#pragma unroll
        for (int hh = 0; hh < NH; ++hh) {
#pragma unroll
            for (int k = 0; k < 4; ++k) r[hh][k] = 0.f;
            if (a.g_emb != nullptr) {
#pragma unroll
                for (int j = 0; j < DV; ++j) {
                    const float gv = a.g_emb[((size_t)b * DM + hh * DV + j) * HW + tl.pix];
#pragma unroll
                    for (int k = 0; k < 4; ++k) r[hh][k] = fmaf(gv, a.Wc[(size_t)(hh * DV + j) * C + c4 + k], r[hh][k]);
                }
            }
        }
        const float* xp = a.x + ((size_t)b * T * C + c4) * HW + tl.pix;
        float* gp = a.gx + ((size_t)b * T * C + c4) * HW + tl.pix;
        for (int t0 = 0; t0 < T; t0 += GX_TC) {
            __syncthreads();
#pragma unroll
            for (int arr = 0; arr < 2; ++arr) {     // rows (array, t, head) = w + 16k: head w of every step
                const float* src = arr ? a.GS : a.attn_in;
                float v[GX_TC];
#pragma unroll
                for (int tt = 0; tt < GX_TC; ++tt)
                    v[tt] = t0 + tt < T ? src[((size_t)(w * a.B + b) * T + t0 + tt) * HW + tl.pix] : 0.f;
#pragma unroll
                for (int tt = 0; tt < GX_TC; ++tt) AGl[((arr * GX_TC + tt) * NH + w) * 64 + lane] = v[tt];      // GGl follows AGl
            }
            __syncthreads();
            for (int tt = 0; tt < GX_TC && t0 + tt < T; ++tt) {
                const int t = t0 + tt;
                float xv[4], dx[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[k] = xp[((size_t)t * C + k) * HW];
#pragma unroll
                for (int hh = 0; hh < NH; ++hh) {
                    const float av = AGl[(tt * NH + hh) * 64 + lane], gv = GGl[(tt * NH + hh) * 64 + lane];
#pragma unroll
                    for (int k = 0; k < 4; ++k) dx[k] = fmaf(av, r[hh][k], fmaf(gv, a.U[hh * C + c4 + k], dx[k]));
                }
                if (tl.act) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float xn = (xv[k] - mean) * rstd;
                        gp[((size_t)t * C + k) * HW] = rstd * (a.gamma[c4 + k] * dx[k] - m1 - xn * m2);
                    }
                }
            }
        }
    }
}

void init_hook() {
    C2S_RAISE_LDS(ltae_long_fwd_kernel<64>);
    C2S_RAISE_LDS(ltae_long_fwd_kernel<128>);
    C2S_RAISE_LDS(ltae_long_fwd_kernel<256>);
    C2S_RAISE_LDS(ltae_long_bwd_heads_kernel<64>);
    C2S_RAISE_LDS(ltae_long_bwd_heads_kernel<128>);
    C2S_RAISE_LDS(ltae_long_bwd_heads_kernel<256>);
    C2S_RAISE_LDS(ltae_long_bwd_vz_kernel<64>);
    C2S_RAISE_LDS(ltae_long_bwd_vz_kernel<128>);
    C2S_RAISE_LDS(ltae_long_bwd_vz_kernel<256>);
    C2S_RAISE_LDS(ltae_long_bwd_gx_kernel);
}
C2sInitRegistrar registrar(init_hook);

}  // namespace

int ltae_long_fwd(const LtaeLongArgs& a, hipStream_t st) {
    C2S_REQUIRE(a.C == 64 || a.C == 128 || a.C == 256, "ltae_long: C must be 64, 128 or 256");
    C2S_REQUIRE(a.attn != nullptr && a.attn_pre != nullptr, "ltae_long_fwd: attn and attn_pre (the score scratch) are required");
    c2s_ensure_init();
    const dim3 grid(ltae_long_tiles(a.B, a.HW));
    if (a.C == 64) hipLaunchKernelGGL(ltae_long_stats_kernel<4>, grid, dim3(1024), 0, st, a);
    else if (a.C == 128) hipLaunchKernelGGL(ltae_long_stats_kernel<8>, grid, dim3(1024), 0, st, a);
    else hipLaunchKernelGGL(ltae_long_stats_kernel<16>, grid, dim3(1024), 0, st, a);
    C2S_CHECK_LAUNCH("ltae_long_stats");
    if (a.C == 64) hipLaunchKernelGGL(ltae_long_fwd_kernel<64>, grid, dim3(1024), HEADS_LDS, st, a);
    else if (a.C == 128) hipLaunchKernelGGL(ltae_long_fwd_kernel<128>, grid, dim3(1024), HEADS_LDS, st, a);
    else hipLaunchKernelGGL(ltae_long_fwd_kernel<256>, grid, dim3(1024), HEADS_LDS, st, a);
    C2S_CHECK_LAUNCH("ltae_long_fwd");
    return C2S_OK;
}

int ltae_long_bwd(const LtaeLongArgs& a, hipStream_t st) {
    C2S_REQUIRE(a.C == 64 || a.C == 128 || a.C == 256, "ltae_long: C must be 64, 128 or 256");
    C2S_REQUIRE(a.attn_in != nullptr, "ltae_long_bwd: attn is required");
    c2s_ensure_init();
    const dim3 grid(ltae_long_tiles(a.B, a.HW));
    if (a.C == 64) hipLaunchKernelGGL(ltae_long_bwd_heads_kernel<64>, grid, dim3(1024), HEADS_LDS, st, a);
    else if (a.C == 128) hipLaunchKernelGGL(ltae_long_bwd_heads_kernel<128>, grid, dim3(1024), HEADS_LDS, st, a);
    else hipLaunchKernelGGL(ltae_long_bwd_heads_kernel<256>, grid, dim3(1024), HEADS_LDS, st, a);
    C2S_CHECK_LAUNCH("ltae_long_bwd_heads");
    if (a.C == 64) hipLaunchKernelGGL(ltae_long_bwd_vz_kernel<64>, grid, dim3(1024), VZ_LDS, st, a);
    else if (a.C == 128) hipLaunchKernelGGL(ltae_long_bwd_vz_kernel<128>, grid, dim3(1024), VZ_LDS, st, a);
    else hipLaunchKernelGGL(ltae_long_bwd_vz_kernel<256>, grid, dim3(1024), VZ_LDS, st, a);
    C2S_CHECK_LAUNCH("ltae_long_bwd_vz");
    if (a.gx == nullptr) return C2S_OK;       // no input gradient: the vz kernel wrote the d gamma / d beta partials
    hipLaunchKernelGGL(ltae_long_bwd_gx_kernel, grid, dim3(1024), GX_LDS, st, a);
    C2S_CHECK_LAUNCH("ltae_long_bwd_gx");
    return C2S_OK;
}
