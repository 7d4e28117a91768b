// The ring design of the 8-wave Winograd convolutions (conv_winograd16.hip, conv_s2wino.hip, conv_s2dgrad.hip): what the three
// share, stated once.
//
// A persistent workgroup of 8 waves per CU walks (frame, tile) pairs t = start, + gridDim.x, ... and skips padded frames.  Its
// operands arrive by LDS-DMA into two rings: U (transformed weights) as five half slabs, one per k-step, a chunk = two of them;
// the raw tile as 3-4 slots of NPLANES planes, one gathered float per lane and piece.  The requests run two chunks ahead of the
// MFMAs (the raw tile, which comes from HBM, three where RAW_AHEAD) and across tile boundaries: the staging side keeps a tile
// cursor of its own (RingCursor) that runs ahead of the tile being multiplied.  One barrier per chunk, in its middle
// (ring_wait_landed).  The frame flags sit as a bit mask in LDS behind the rings, so the walk never touches the vector-memory
// counter, which orders the requests in flight.
//
//   all four (conv_winograd.hip too):  ring_check, ring_grid, the padding rule (tile_pixel_offset of conv_tile.h), the
//                                       address-space macros and the vector typedefs
//   the three 8-wave kernels:          RingGeom, ring_frame_flags, RingWalk, ring_stage_raw, RingCursor, ring_wait_landed,
//                                       ring_load_a, ring_load_d, ring_opaque, ring_store_rows, ring_lds_bytes, ring_max_frames
//   conv_winograd16, conv_s2wino:      ring_stage_u
//   conv_s2wino:                       ring_gather
//
// Each kernel keeps its pixel map (the functor of ring_gather), transforms, adjoint folds, MFMA schedule (kstep / chunk), output
// transform, and conv_s2dgrad its skip epilogue.  conv_winograd.hip (4 waves, register staging, double buffer) is another loop.
// The rule for a shared device piece is conv_tile.h's: it goes in where the default build keeps the kernel's registers, scratch,
// occupancy and static instruction counts, and its time.  conv_s2dgrad, which sits at 256 VGPRs with 16 / 32 bytes of scratch,
// keeps its own gather table and U requests: through the shared ones it came out with 20-40 bytes and a spill inside the chunk
// loop.  conv_winograd16 keeps its own gather table: through ring_gather its forward launches ran 1.0-1.7 % slower
// (profiles/conv_ring_refactor.txt).
#pragma once
#include "conv_tile.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#define C2S_AS1 __attribute__((address_space(1)))
#define C2S_AS3 __attribute__((address_space(3)))

// a buffer offset that is out of range whatever scalar offset joins it: reads as 0, is not stored (frames stay below it: ring_check)
constexpr int RING_OOB = 0x7FFF0000;

// ------------------------------------------------------------------------------------------------------------------ geometry
// LDS of one kernel, in floats: | U ring: 5 half slabs | raw ring: XSLOTS slots | bias of the block's 64 channels, if any | frame
// flag bits.  A raw slot holds NPLANES planes (RR rows of pitch RC) at pitch XP (= 32 mod 64 banks: the four k groups of a wave
// do not collide) and a zero-filled tail up to MAXE floats per thread.
template <int UHALF_, int XSLOTS_, int NPLANES_, int RR_, int RC_, int XP_, int BIAS_FLOATS_>
struct RingGeom {
    static constexpr int UHALF = UHALF_, USLAB = 2 * UHALF, URING = 5 * UHALF;      // a k-step's half slab; a chunk; the ring
    static constexpr int UPIECES = USLAB / 4 / 512;                                 // 16-byte LDS-DMA pieces per thread and chunk
    static constexpr int XSLOTS = XSLOTS_, NPLANES = NPLANES_, RR = RR_, RC = RC_, PLANE = RR * RC, XP = XP_;
    static constexpr int MAXE = (NPLANES * XP + 511) / 512;                         // one-float pieces per thread and raw slot
    static constexpr int XS = MAXE * 512;                                           // floats per raw slot
    static constexpr int BIAS = URING + XSLOTS * XS;                                // where the bias sits
    static constexpr int FLAGS = BIAS + BIAS_FLOATS_;                               // where the flag bits sit = floats before them
    static_assert(USLAB % 2048 == 0 && XP >= PLANE && XP % 64 == 32 && MAXE < 16, "whole pieces; bank pitch; vmcnt(MAXE)");
};
// frames of one launch: their flag bits share what the rings leave of the 160 KB of LDS; the walk counts tiles in an int
template <class G>
constexpr int ring_max_frames() {
    return 32 * (160 * 1024 / 4 - G::FLAGS) < 65536 ? 32 * (160 * 1024 / 4 - G::FLAGS) : 65536;
}
template <class G>
static inline size_t ring_lds_bytes(int N) {
    return (size_t)(G::FLAGS + (N + 31) / 32) * sizeof(float);
}

// ---------------------------------------------------------------------------------------------------------------- the walk
// valid[N] -> bit mask at `flags` (a barrier must follow)
__device__ __forceinline__ void ring_frame_flags(unsigned* flags, const int* valid, int N, int tid) {
    for (int wi = tid; wi < (N + 31) / 32; wi += 512) {
        unsigned m = 0;
        for (int b = 0; b < 32; ++b) {
            const int f = wi * 32 + b;
            if (f < N && (valid == nullptr || valid[f] != 0)) m |= 1u << b;
        }
        flags[wi] = m;
    }
}
struct RingWalk {
    const unsigned* flags;
    int ntotal, tiles, tiles_x;          // N * tiles; tiles per frame; per tile row
    // the first tile at or after tt (in steps of the grid) whose frame is real; >= ntotal: none
    __device__ __forceinline__ int next_valid(int tt) const {
        while (tt < ntotal) {
            const int f = tt / tiles;
            if ((flags[f >> 5] >> (f & 31)) & 1u) break;
            tt += gridDim.x;
        }
        return tt;
    }
    // XCD-aware start: each XCD walks a contiguous eighth of the tiles in flight
    __device__ __forceinline__ int first() const { return next_valid((int)C2S_XCD_ORDER(blockIdx.x, gridDim.x)); }
    // frame and first pixel of tile tt, tiles of TH x TW pixels
    template <int TH, int TW>
    __device__ __forceinline__ void origin(int tt, int& n, int& y0, int& x0) const {
        n = tt / tiles;
        const int ti = tt - n * tiles;
        const int tyi = ti / tiles_x, txi = ti - tyi * tiles_x;
        y0 = tyi * TH; x0 = txi * TW;
    }
};

// ----------------------------------------------------------------------------------------------------------------- staging
// The gather table of a tile: LDS float e = tid + 512 i of a raw slot is element (row r, column q) of plane pl; map(pl, r, q, c,
// gy, gx) names its source channel (within the chunk) and pixel and returns false for an element the kernel does not use.
// goff[i] = byte offset within the frame's first chunk, RING_OOB for padding, tile overhang and the tail.
template <class G, class Map>
__device__ __forceinline__ void ring_gather(int (&goff)[G::MAXE], int tid, int H, int W, int pad_mode, Map map) {
#pragma unroll
    for (int i = 0; i < G::MAXE; ++i) {
        const int e = tid + i * 512;
        const int pl = e / G::XP, rem = e - pl * G::XP;
        const int r = rem / G::RC, q = rem - r * G::RC;
        int c, gy, gx;
        const bool used = map(pl, r, q, c, gy, gx) && rem < G::PLANE && pl < G::NPLANES;
        const int px = tile_pixel_offset(gy, gx, H, W, 1, 1, pad_mode);
        goff[i] = used && px >= 0 ? (c * H * W + px) * 4 : RING_OOB;
    }
}
// U chunk at g (USLAB floats, contiguous, packed lane-linear) -> half slabs h0 and h0 + 1 (mod 5).  Piece i of wave w covers
// floats 2048 i + 256 w ..; a half slab that is no whole number of pieces (conv_s2wino: 1.5) splits one at a wave boundary.
// LDS destinations are wave-uniform and stay in scalar registers (w: the wave, scalar).
template <class G>
__device__ __forceinline__ void ring_stage_u(float* lds, const C2S_AS1 char* g, int h0, int w, int tid) {
    const int h1 = h0 == 4 ? 0 : h0 + 1;
    float* d0 = lds + h0 * G::UHALF + w * 256;
    float* d1 = lds + h1 * G::UHALF + w * 256;
#pragma unroll
    for (int i = 0; i < G::UPIECES; ++i) {
        const bool second = G::UHALF % 2048 == 0 ? i * 2048 >= G::UHALF : i * 2048 + w * 256 >= G::UHALF;
        __builtin_amdgcn_global_load_lds((const C2S_AS1 void*)(g + i * 8192 + (unsigned)(tid * 16)), (C2S_AS3 void*)(second ? d1 + (i * 2048 - G::UHALF) : d0 + i * 2048), 16, 0, 0);
    }
}
// the chunk's planes of the tile -> raw slot: MAXE one-float pieces, the chunk's channel offset chan0 scalar
template <class G>
__device__ __forceinline__ void ring_stage_raw(float* lds, __amdgpu_buffer_rsrc_t r, const int (&goff)[G::MAXE], int chan0, int slot, int w) {
    float* Xd = lds + G::URING + slot * G::XS + w * 64;
#pragma unroll
    for (int i = 0; i < G::MAXE; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (C2S_AS3 void*)(Xd + i * 512), 4, goff[i], chan0, 0, 0);
}
// The request cursor (uniform across the workgroup): chunk sk of tile stile is the next to request; stile >= ntotal: none left.
// request(h0, slot) issues one chunk's requests and moves on; at a tile's last chunk it walks to the next real tile and calls
// begin(tile) (the gather table and the frame's buffer resource).  RAW_AHEAD: the raw tile is requested a chunk before its U
// (three chunks ahead of the MFMAs, U two), so request() sends the U chunk of the raw request before (u_ok, u_k) and then the
// next raw tile; the first call primes the raw side alone.  young_raw: the youngest MAXE requests in flight are raw pieces of
// the chunk after next, which the chunk barrier need not wait for.
template <bool RAW_AHEAD>
struct RingCursor {
    int stile, sk = 0, u_k = 0;
    bool u_ok = false, young_raw = false;
    template <class Begin, class StageU, class StageRaw>
    __device__ __forceinline__ void request(const RingWalk& wk, int K, int h0, int slot, Begin begin, StageU stage_u, StageRaw stage_raw) {
        if constexpr (RAW_AHEAD) {
            if (u_ok) stage_u(u_k, h0);
            u_ok = stile < wk.ntotal;
            u_k = sk;
            young_raw = u_ok;
            if (!u_ok) return;
        } else {
            if (stile >= wk.ntotal) return;
            stage_u(sk, h0);
        }
        stage_raw(sk, slot);
        if (++sk == K) {                               // once per multiplied tile
            sk = 0;
            stile = wk.next_valid(stile + gridDim.x);
            if (stile < wk.ntotal) begin(stile);
        }
    }
};
// in front of the chunk barrier: everyone's requests for the NEXT chunk have landed (loads complete in order)
template <class G>
__device__ __forceinline__ void ring_wait_landed(bool young_raw) {
    if (young_raw) __builtin_amdgcn_s_waitcnt(0x0F70 | G::MAXE);       // vmcnt(MAXE)
    else __builtin_amdgcn_s_waitcnt(0x0F70);                           // vmcnt(0)
    __builtin_amdgcn_s_barrier();
}

// ---------------------------------------------------------------------------------------------------------- operand reads
// A operand: PIECES ds_read_b128, STRIDE floats apart
template <int PIECES, int STRIDE>
__device__ __forceinline__ void ring_load_a(const float* ab, float (&a)[4 * PIECES]) {
#pragma unroll
    for (int q4 = 0; q4 < PIECES; ++q4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(ab + q4 * STRIDE);
        a[4 * q4] = v[0]; a[4 * q4 + 1] = v[1]; a[4 * q4 + 2] = v[2]; a[4 * q4 + 3] = v[3];
    }
}
// ROWS patch rows of pitch RC as (cols 0,1), (cols 2,3)
template <int ROWS, int RC>
__device__ __forceinline__ void ring_load_d(const float* bb, f32x2 (&dl)[ROWS], f32x2 (&dh)[ROWS]) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        dl[r] = *reinterpret_cast<const f32x2*>(bb + r * RC);
        dh[r] = *reinterpret_cast<const f32x2*>(bb + r * RC + 2);
    }
}
// the lane's raw-slot offsets of the two k-steps, opaque: the row offsets then stay ds_read2 immediates
__device__ __forceinline__ void ring_opaque(int& boff0, int& boff1) { asm volatile("" : "+v"(boff0), "+v"(boff1)); }

// ------------------------------------------------------------------------------------------------------------------ epilogue
// y[channel of a pair][output row] (V = f32x2: 8-byte rows, f32x4: 16-byte rows) -> out at vector offsets vo0 / vo1 (the rows;
// RING_OOB outside the plane) + scalar offset so + channel * cstride.  Accumulation: the four reads in flight before the first add.
template <class V>
__device__ __forceinline__ V ring_row_load(__amdgpu_buffer_rsrc_t ro, int vo, int so) {
    if constexpr (sizeof(V) == 8) return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(ro, vo, so, 0));
    else return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(ro, vo, so, 0));
}
template <class V>
__device__ __forceinline__ void ring_store_rows(__amdgpu_buffer_rsrc_t ro, int vo0, int vo1, int so, int cstride, int accumulate, V (&y)[2][2]) {
    if (accumulate) {
        V o[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            o[j][0] = ring_row_load<V>(ro, vo0, so + j * cstride);
            o[j][1] = ring_row_load<V>(ro, vo1, so + j * cstride);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            y[j][0] += o[j][0];
            y[j][1] += o[j][1];
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (sizeof(V) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, y[j][i]), ro, i == 0 ? vo0 : vo1, so + j * cstride, 0);
            else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y[j][i]), ro, i == 0 ? vo0 : vo1, so + j * cstride, 0);
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- host side
// The descriptor checks every Winograd convolution makes, under the entry point's name: required pointers, at most max_frames
// frames, a dense output, and frames within 32-bit byte offsets: a source frame below src_limit and, where the kernel stores
// through buffer offsets (out_offsets), an output frame below RING_OOB.
static inline int ring_check(const char* who, const c2s_conv_desc* d, bool pointers, int max_frames, long src_limit, bool out_offsets) {
    C2S_REQUIRE(d && pointers, "%s: null pointer", who);
    C2S_REQUIRE(d->N > 0 && d->N <= max_frames, "%s: more than %d frames in one launch (N = %d)", who, max_frames, d->N);
    C2S_REQUIRE(d->OutH == d->Hout && d->OutW == d->Wout && d->osy == 1 && d->osx == 1 && d->ooy == 0 && d->oox == 0,
                "%s: dense output only", who);
    C2S_REQUIRE((long)(d->C0 > d->C1 ? d->C0 : d->C1) * d->Hin * d->Win * 4 < src_limit &&
                (!out_offsets || (long)d->CoutP * d->Hout * d->Wout * 4 < RING_OOB), "%s: frame too large", who);
    return C2S_OK;
}
// persistent grid: per_cu workgroups per CU, split over the yblocks output-channel (and parity) blocks, at most one per tile
static inline dim3 ring_grid(int yblocks, long ntotal, int per_cu) {
    long gx = ((long)per_cu * c2s_cus() + yblocks - 1) / yblocks;      // (c2s_cus runs the init hooks: dynamic LDS limit)
    if (gx > ntotal) gx = ntotal;
    return dim3((unsigned)gx, yblocks, 1);
}
