// The 32x32-MFMA tile design of the implicit-GEMM convolutions (conv_igemm.hip, conv_xpair.hip, conv_bf16x3.hip): what the three
// share, and the device pieces conv_igemm's kernel is built from.
//
// A workgroup owns NF position fragments of 32 positions each (FR rows x FC columns, FC = 2^log2fc adapts to narrow planes:
// 128 -> 1x32, 16 -> 2x16) by 32*MF output channels.  MFMA rows are output channels, MFMA columns are positions, so lanes 0..31
// of a store hit 32 consecutive x of one NCHW row.  The input tile (halo included) and the weight slab of a chunk of CK input
// channels go to registers through buffer loads and from there to LDS, double-buffered; the operand reads of the MFMAs run LA
// k-steps ahead.
//
//   all three:   tile_log2fc, tile_count, tile_lane, TileParams, tile_check, tile_fill; tile_lds_bytes, tile_wide, tile_frame_order
//                (conv_igemm, conv_xpair); tile_pixel_offset (conv_igemm, conv_bf16x3)
//   conv_igemm:  TileStage (offsets / prefetch / commit), tile_chunk_loop, tile_store
//
// conv_xpair (float2 stores, two weight operands per k-step) and conv_bf16x3 ([position][8 channels] bf16 staging, three MFMAs
// per product) keep their own staging, loop and epilogue: each ran slower through the pieces below (profiles/conv_tile_refactor.txt).
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------------------------ geometry
// log2 of the fragment width FC for an output plane Wout wide (FR = 32 >> log2fc rows per fragment)
__host__ __device__ inline int tile_log2fc(int Wout) {
    int l2 = 5;
    while (l2 > 2 && (1 << l2) > Wout) --l2;
    return l2;
}
// tiles of nf position fragments that cover an Hout x Wout plane (tiles_x of them per tile row)
static inline int tile_count(int Hout, int Wout, int log2fc, int nf) {
    return cdiv(Wout, 1 << log2fc) * cdiv(Hout, nf * (32 >> log2fc));
}
// floats of one LDS buffer [CK][plane] | weights (the weights start 16-byte aligned), and the bytes of the double-buffered pair
__host__ __device__ constexpr int tile_x_floats(int ck, int plane) { return (ck * plane + 3) & ~3; }
__host__ __device__ constexpr int tile_buf_floats(int ck, int plane, int wfloats) { return tile_x_floats(ck, plane) + wfloats; }
static inline size_t tile_lds_bytes(int ck, int plane, int wfloats) { return 2 * (size_t)tile_buf_floats(ck, plane, wfloats) * sizeof(float); }
// 64-channel tiles halve the LDS reads per MFMA, but on small planes (16x16 and below) they leave the grid short of two
// workgroups per CU: 32-channel tiles there
static inline bool tile_wide(int CoutP, int tiles, int N, int cus) {
    return CoutP % 64 == 0 && (long)tiles * N * (CoutP / 64) >= 2L * cus;
}

// lane -> MFMA column li (position of the fragment: row fy, column fx) and k half lk
struct TileLane {
    int li, lk, fy, fx;
};
__device__ __forceinline__ TileLane tile_lane(int tid, int log2fc) {
    const int lane = tid & 63, li = lane & 31;
    return {li, lane >> 5, li >> log2fc, li & ((1 << log2fc) - 1)};
}

// ------------------------------------------------------------------------------------------------------ (frame, tile) order
// XCD-aware placement (workgroups go to the 8 XCDs round-robin in linear order): each XCD takes a contiguous eighth of the
// (frame, tile) range, so tiles that share halo rows are processed behind the same L2.  Only where one workgroup covers all
// output channels and the range divides by 8 (C2S_XCD_ORDER is the identity otherwise: tested here to skip the division).
__device__ __forceinline__ void tile_frame_order(int& bxi, int& n) {
    bxi = blockIdx.x, n = blockIdx.z;
    const unsigned tot = gridDim.x * gridDim.z;
    if (gridDim.y == 1 && (tot & 7) == 0) {
        const unsigned l = C2S_XCD_ORDER(blockIdx.x + gridDim.x * blockIdx.z, tot);
        n = (int)(l / gridDim.x);
        bxi = (int)(l - (unsigned)n * gridDim.x);
    }
}

// ------------------------------------------------------------------------------------------------------------------- staging
// Element index within a plane of input pixel (gy, gx) under zero or single-reflection padding; -1 = reads as zero (padding,
// or beyond the padded plane: positions of a ragged tile)
__device__ __forceinline__ int tile_pixel_offset(int gy, int gx, int Hin, int Win, int pad_y, int pad_x, int pad_mode) {
    bool ok;
    if (pad_mode == C2S_PAD_REFLECT) {
        ok = gy >= -pad_y && gy < Hin + pad_y && gx >= -pad_x && gx < Win + pad_x;
        gy = reflect_idx(gy, Hin);
        gx = reflect_idx(gx, Win);
    } else {
        ok = gy >= 0 && gy < Hin && gx >= 0 && gx < Win;
    }
    return ok ? gy * Win + gx : -1;
}

// Global -> register -> LDS staging of one chunk: CK channels of a rows x cols input tile as [CK][plane], and the weight slab
// [NSLAB][CK][COT] out of wpk[NSLAB][Cin][CoutP].  The channels are the concatenation of two sources (a chunk never straddles
// them: the host checks C0 % CK == 0 when C1 > 0).
// Buffer loads: out-of-range offsets (padding = -1, channels beyond Cin, idle lanes) return 0 in hardware, so no select
// follows the load and the wait can sink to the LDS commit.
template <int CK_, int MAXE, int NTHR, int NSLAB, int COT>
struct TileStage {
    static constexpr int CK = CK_;
    static constexpr int WV = COT / 4;                  // float4 per (slab, channel) weight row
    static constexpr int NWV = NSLAB * CK * WV;         // float4 items of the weight slab
    static constexpr int WPT = (NWV + NTHR - 1) / NTHR;
    static constexpr int WFLOATS = NSLAB * CK * COT;

    int goff[MAXE];                                     // byte offsets within a frame, relative to the chunk's first channel
    float xr[MAXE];
    f32x4 wr[WPT];
    __amdgpu_buffer_rsrc_t r0, r1, rw;
    int tid, total, C0, Cin, HWin, CoutP, co0;

    // (gy0, gx0) = input pixel of the tile's first staged element; reflection is resolved here, once per tile
    __device__ __forceinline__ void init(int tid_, int n, const float* src0, const float* src1, const float* wpk, int C0_, int C1,
                                         int Hin, int Win, int CoutP_, int co0_, int plane, int cols, int gy0, int gx0, int pad_y,
                                         int pad_x, int pad_mode) {
        tid = tid_; C0 = C0_; Cin = C0_ + C1; HWin = Hin * Win; CoutP = CoutP_; co0 = co0_;
        total = CK * plane;
#pragma unroll
        for (int i = 0; i < MAXE; ++i) {
            const int e = tid + i * NTHR;
            int off = -1;
            if (e < total) {
                const int c = e / plane;
                const int rem = e - c * plane;
                const int r = rem / cols;
                const int px = tile_pixel_offset(gy0 + r, gx0 + rem - r * cols, Hin, Win, pad_y, pad_x, pad_mode);
                if (px >= 0) off = (c * HWin + px) * 4;
            }
            goff[i] = off;
        }
        const float* s0n = src0 + (size_t)n * C0 * HWin;
        r0 = __builtin_amdgcn_make_buffer_rsrc((void*)s0n, 0, C0 * HWin * 4, 0x00020000);
        const float* s1n = src1 != nullptr ? src1 + (size_t)n * C1 * HWin : s0n;
        r1 = __builtin_amdgcn_make_buffer_rsrc((void*)s1n, 0, C1 * HWin * 4, 0x00020000);
        rw = __builtin_amdgcn_make_buffer_rsrc((void*)wpk, 0, NSLAB * Cin * CoutP * 4, 0x00020000);
    }

    __device__ __forceinline__ void prefetch(int cb) {
        const bool first = cb < C0;
        const int chan0 = (first ? cb : cb - C0) * HWin * 4;
        if (first) {
#pragma unroll
            for (int i = 0; i < MAXE; ++i)
                xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r0, goff[i] >= 0 ? goff[i] + chan0 : -1, 0, 0));
        } else {
#pragma unroll
            for (int i = 0; i < MAXE; ++i)
                xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r1, goff[i] >= 0 ? goff[i] + chan0 : -1, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int e = tid + i * NTHR;
            const int o4 = e % WV, tc = e / WV;
            const int c = tc % CK, t = tc / CK;
            const bool ok = e < NWV && cb + c < Cin;
            const int off = ok ? (((t * Cin + cb + c) * CoutP + co0 + o4 * 4) * 4) : -1;
            wr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, off, 0, 0));
        }
    }

    __device__ __forceinline__ void commit(float* Xd, float* Wd) const {
#pragma unroll
        for (int i = 0; i < MAXE; ++i) {
            const int e = tid + i * NTHR;
            if (e < total) Xd[e] = xr[i];
        }
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            const int e = tid + i * NTHR;
            if (e < NWV) *reinterpret_cast<f32x4*>(Wd + (size_t)e * 4) = wr[i];
        }
    }
};

// ------------------------------------------------------------------------------------------------------------ the chunk loop
// K loop over the input channels in chunks of Stage::CK, LDS double-buffered ([2][ X | W ], `buf` floats each, W at Wl): one
// barrier per chunk.  While chunk k is multiplied out of buffer k&1, the registers holding chunk k+1 (requested one chunk
// earlier) are committed to the other buffer and the request for chunk k+2 is issued, both in the middle of the MFMA sequence
// (k-step COMMIT_AT of NS) so that neither sits next to the barrier.
// load_ops(Xc, Wc, s, ops) reads the operands of k-step s into an Ops; mfma(ops) issues the MFMAs of one k-step.
template <int NS, int LA, int COMMIT_AT, class Ops, class Stage, class LoadOps, class Mfma>
__device__ __forceinline__ void tile_chunk_loop(Stage& st, float* Xl, float* Wl, int buf, LoadOps load_ops, Mfma mfma) {
    constexpr int CK = Stage::CK;
    const int Cin = st.Cin;
    st.prefetch(0);
    st.commit(Xl, Wl);
    if (CK < Cin) st.prefetch(CK);
    __syncthreads();
    int cur = 0;
    for (int cb = 0; cb < Cin; cb += CK, cur ^= 1) {
        const float* Xc = Xl + cur * buf;
        const float* Wc = Wl + cur * buf;
        Ops ops[LA + 1];
#pragma unroll
        for (int s_ = 0; s_ < LA; ++s_) load_ops(Xc, Wc, s_, ops[s_]);
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) {
            // operands LA k-steps ahead; the scheduling barriers keep hipcc from sinking the ds_reads below the
            // MFMAs that hide them (it would then wait on them right away) or hoisting a whole chunk's reads
            if (s_ + LA < NS) load_ops(Xc, Wc, s_ + LA, ops[(s_ + LA) % (LA + 1)]);
            __builtin_amdgcn_sched_barrier(0);
            mfma(ops[s_ % (LA + 1)]);
            __builtin_amdgcn_sched_barrier(0);
            if (s_ == COMMIT_AT && cb + CK < Cin) {
                st.commit(Xl + (cur ^ 1) * buf, Wl + (cur ^ 1) * buf);
                if (cb + 2 * CK < Cin) st.prefetch(cb + 2 * CK);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------ epilogue
// Stores the MF accumulator fragments of one position: accumulator element r of channel fragment m is channel
// co0 + 32 m + (r&3) + 8 (r>>2) + 4 lk; get(m, r) returns it; it goes to on[co * chs + sp] (sp = the position within a channel of
// chs floats).  Per element: acc + bias + old.  Accumulation puts eight reads in flight, then their adds and stores --
// read-add-store per element serialised 32 memory round trips (the compiler cannot move a read above the store before it).
template <int MF, class Get>
__device__ __forceinline__ void tile_store(float* on, size_t sp, size_t chs, int co0, int lk, int Cout, const float* bias, int accumulate,
                                           Get get) {
#pragma unroll
    for (int m = 0; m < MF; ++m) {
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 8) {
            float old[8];
            if (accumulate) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int r = r0 + u;
                    const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                    old[u] = co < Cout ? on[(size_t)co * chs + sp] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = r0 + u;
                const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (co < Cout) {
                    float v = get(m, r);
                    if (bias != nullptr) v += bias[co];
                    if (accumulate) v += old[u];
                    on[(size_t)co * chs + sp] = v;
                }
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- host side
struct TileParams {
    const float* src0;
    const float* src1;
    const float* wpk;
    const float* bias;
    float* out;
    const int* valid;
    int C0, C1, Hin, Win, Cout, CoutP, Hout, Wout, OutH, OutW;
    int pad_y, pad_x, pad_mode, osy, osx, ooy, oox, accumulate;
    int log2fc, tiles_x;
    // reflect adjoint (data gradient of a reflect-padded convolution).  Per dimension the fold of the halo gradient
    // is:  operand(pos == lo, tap K-1) += input[tap position - d_lo]   and
    //      operand(pos == hi, tap 0)   += input[tap position + d_hi]      (-1 = rule absent; d = K-1 except in the
    //      parity sub-kernels of the 6x6 stride-2 data gradient, where the mirrored row is one or two rows away)
    int adj, ay_lo, ay_hi, ax_lo, ax_hi;
    int dy_lo, dy_hi, dx_lo, dx_hi;
};

// The descriptor checks every tile kernel makes, under the entry point's name; `pointers` = its required pointers are all set
static inline int tile_check(const char* who, const c2s_conv_desc* d, bool pointers) {
    C2S_REQUIRE(d && pointers, "%s: null pointer", who);
    C2S_REQUIRE(d->CoutP % 32 == 0 && d->CoutP >= d->Cout, "%s: CoutP must be a multiple of 32", who);
    C2S_REQUIRE(d->N <= C2S_CONV_MAX_FRAMES, "%s: more than 65535 frames in one launch (N = %d): the frame index is gridDim.z", who, d->N);
    C2S_REQUIRE((long)(d->C0 > d->C1 ? d->C0 : d->C1) * d->Hin * d->Win * 4 < (1L << 31), "%s: frame too large", who);
    return C2S_OK;
}

// The descriptor as kernel parameters, with the fragment width of its output plane and no adjoint rule
static inline void tile_fill(TileParams& p, const c2s_conv_desc* d, const float* src0, const float* src1, const float* wpk,
                             const float* bias, float* out, const int* valid) {
    p.src0 = src0; p.src1 = src1; p.wpk = wpk; p.bias = bias; p.out = out; p.valid = valid;
    p.C0 = d->C0; p.C1 = d->C1; p.Hin = d->Hin; p.Win = d->Win; p.Cout = d->Cout; p.CoutP = d->CoutP;
    p.Hout = d->Hout; p.Wout = d->Wout; p.OutH = d->OutH; p.OutW = d->OutW;
    p.pad_y = d->pad_y; p.pad_x = d->pad_x; p.pad_mode = d->pad_mode;
    p.osy = d->osy; p.osx = d->osx; p.ooy = d->ooy; p.oox = d->oox; p.accumulate = d->accumulate;
    p.log2fc = tile_log2fc(d->Wout);
    p.tiles_x = cdiv(d->Wout, 1 << p.log2fc);
    p.adj = d->reflect_adjoint;
    p.ay_lo = p.ay_hi = p.ax_lo = p.ax_hi = -1;
    p.dy_lo = p.dy_hi = p.dx_lo = p.dx_hi = d->KH - 1;
}
