// 3x3 stride-1 pad-1 convolution (forward and data gradient) as Winograd F(2x2, 3x3) on v_mfma_f32_16x16x4_f32, with the
// OUTPUT TRANSFORM IN REGISTERS: every lane holds all 16 transform-domain values of its (output channels, 2x2 block), so the
// epilogue needs no exchange between waves.
//
//   Y(2x2 block) = At [ (G g Gt) (.) (Bt d B) ] A        M[p][o][t] = sum_c U[p][c][o] * V[p][c][t],  p = 4 xi + nu
//
// conv_winograd.hip gives wave xi one ROW of the 4x4 transform domain (8 accumulators of 32x32), so the xi-sum of the output
// transform crosses waves: three LDS barriers and a 64 KB exchange per tile (10.5 k of its 56 k cycles per tile, with the MFMA
// pipe of that workgroup idle; tools/wino_stamps.py).  Here a wave owns all 16 points of 32 OUTPUT CHANNELS x 16 BLOCKS:
//   workgroup = 8 waves on one tile of 64 blocks x 64 output channels; wave w: channels 32 (w & 1) .., 16 blocks of one block
//   row;  accumulators acc[16 points][2 channel groups] of 16x16 = 128 VGPRs.  The tile is 4 x 16 blocks = 8 x 32 output pixels
//   (template BR x BC; 2 x 32 was measured and is not instantiated, see the launch).
//   A operand = U[p][c][o]   lane (o = lane & 15, k = lane >> 4): four ds_read_b128, one per row xi of the 4x4 points; a half slab
//                            is stored [c][xi][o][nu], so the 16 lanes of a read touch 256 contiguous bytes
//   B operand = V[p][c][t]   lane (t = lane & 15 = block column, k = lane >> 4) transforms the WHOLE 4x4 patch of its (block,
//                            channel): four ds_read2_b64, 16 packed VALU ops (v_pk_add_f32), used by 32 MFMAs
//   D                        lane (t, q): channels 4q .. 4q+3 of block t, for all 16 points -> At M A in registers, one float2
//                            per output row (16 lanes = 128 contiguous bytes)
// tools/_diag/mfma_rate.hip: on this chip every VALU instruction of a wave costs the SIMD ~8 cycles of MFMA issue (a 16x16x4
// fp32 MFMA is 32), whichever wave it comes from -- so the budget is VALU instructions per MFMA: 0.5 here (a first version
// with 16 channels x 32 blocks per wave and scalar adds had 2.5 and ran at the 4-wave kernel's speed).
// Operands arrive by LDS-DMA (U: global_load_lds_dwordx4 of a slab packed lane-linear; raw tile: buffer_load_dword ... lds,
// one gathered float per lane) into THREE buffers: the requests run two chunks ahead of the MFMAs across tile boundaries, and
// the single barrier per chunk sits in its middle, so no wave waits at a barrier for data and the first operand reads of a
// chunk are in flight during the last MFMAs of the chunk before.  Persistent workgroups, one per CU.
// Data gradient of the reflect-padded convolution: the adjoint folds onto the raw patch of the border blocks (top: d3 += d1,
// bottom: d0 += d2, left: col3 += col1, right: col0 += col2), only in the waves / tiles that touch a border (uniform branches).
//
// Reference call sites replaced: as conv_winograd.hip (nn.Conv2d 3x3: src/backbones/conv.py:70-80,378-382 and its
// convolution_backward-input incl. reflection_pad2d_backward).  Planes at least 32 pixels wide; narrower ones stay with the
// 4-wave kernel.
#include "conv_ring.h"
#include <stdlib.h>

namespace {

#ifdef C2S_W16_STAMP
// diagnostic build only (tools/wino16_diag.py --stamps): per workgroup, cycles wave 0 spent between the top of the s_waitcnt in
// front of the chunk barrier and the instruction after the barrier, the kernel's total, the number of chunks, and the cycles of
// the epilogues
__device__ unsigned long long w16_stamps[1024 * 4];
#endif

struct Wino16Params {
    const float* src0;
    const float* src1;
    const float* upk;      // [cout block][chunk][8 c][4 xi][64 o][4 nu]
    const float* bias;
    float* out;
    const int* valid;
    int C0, C1, H, W, Cout, CoutP;
    int pad_mode, accumulate;
    int N, tiles, tiles_x, nchunks;
};

// tile of BR x BC blocks of 2 x 2 output pixels (BR * BC = 64: one block row of 16 blocks per wave and channel half).  A k-step = 4
// channels: a half slab of 4,096 floats = 16 KB of U; a chunk of 8: 32 KB, four 16-byte pieces per thread; raw ring of four slots
// of the chunk's 8 channels; the bias of the 64 channels
template <int BR, int BC>
struct W16Shape {
    static_assert(BR * BC == 64 && BC % 16 == 0, "eight waves: 2 channel halves x BR block rows x BC / 16 column groups");
    static constexpr int RR = 2 * BR + 2, RC = 2 * BC + 2;          // raw tile: 10 x 34 (4 x 16 blocks), 6 x 66 (2 x 32)
    static constexpr int XP = (RR * RC + 31) / 64 * 64 + 32;        // LDS pitch per channel >= the plane (340 / 396): 352 / 416
    using G = RingGeom<W16_CK / 2 * 64 * W16_UP, 4, W16_CK, RR, RC, XP, 64>;      // MAXE 6 / 7: 131,328 / 139,520 B (+ frame flag bits)
};

// tools/wino16_diag.py builds diagnostic copies with one part of the kernel removed (results are then wrong by design):
//   1 = no MFMA, 2 = no staging after the first two chunks, 3 = no output stores, 4 = no LDS operand reads in the K loop,
//   5 = 2 and 4 together (MFMA + transform + epilogue only), 6 = 5 without the barrier per chunk, 7 = 5 without the transforms,
//   8 = no raw-tile staging, 9 = no U staging, 10 = every raw tile from frame 0 (L2 hits), 11 = 7 without the epilogue,
//   12 = 11 without the barrier per chunk (the MFMA loop and the tile walk alone), 13 = raw rows shifted by one float onto a
//   128-byte line (one line less per row), 14 = raw rows of exactly one line
#ifndef C2S_W16_DIAG
#define C2S_W16_DIAG 0
#endif
#define C2S_W16_BARE (C2S_W16_DIAG == 11 || C2S_W16_DIAG == 12)       // 7-like: nothing but MFMAs in the K loop

// a - b - c on channel pairs as two v_pk_add_f32 with negated second operands (the compiler leaves vector subtractions
// scalar).  Only used after the s_nop block that follows the K loop: asm operands are invisible to the MFMA -> VALU hazard
// recogniser.
__device__ __forceinline__ f32x2 sub2(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]\n\tv_pk_add_f32 %0, %0, %3 neg_lo:[0,1] neg_hi:[0,1]"
        : "=&v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

template <bool ADJ, int BR, int BC>
__global__ __launch_bounds__(512, 1) void conv_winograd16_kernel(Wino16Params p) {
    using G = typename W16Shape<BR, BC>::G;
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);    // (scalar: row masks and bases in SGPRs)
    const int t = lane & 15, kq = lane >> 4;        // block column / k index (B, D: channel quad) ; A: output channel / k index
    const int ch = w & 1, brow = (w >> 1) % BR, bcol0 = 16 * ((w >> 1) / BR);      // channel half (32), block row and first block
                                                                                  // column of this wave
    const int co0 = blockIdx.y * 64;
    const int HW = p.H * p.W;
    const int K = p.nchunks;

    const RingWalk walk = {reinterpret_cast<unsigned*>(lds + G::FLAGS), p.N * p.tiles, p.tiles, p.tiles_x};
    ring_frame_flags(reinterpret_cast<unsigned*>(lds + G::FLAGS), p.valid, p.N, tid);
    __syncthreads();
#ifdef C2S_W16_STAMP
    unsigned long long st_wait = 0, st_epi = 0, st_chunks = 0, st_first = 0;
    const unsigned long long st_begin = __builtin_amdgcn_s_memtime();
#endif

    // ---- the staging side runs ahead of the MFMAs, across tile boundaries: its own tile state.  Raw tile element (c, r, q) is
    // input pixel (oy0 - 1 + r, ox0 - 1 + q) of the chunk's channel c
    int goff[G::MAXE];
    int diag_staged = 0;
    __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.src0, 0, 0, 0x00020000), r1 = r0;
    auto begin_staging = [&](int tt) {
        int n, oy0, ox0;
        walk.origin<2 * BR, 2 * BC>(tt, n, oy0, ox0);
        if (C2S_W16_DIAG == 10) n = 0;
        if (C2S_W16_DIAG >= 100) n %= (C2S_W16_DIAG - 100);       // 100 + F: raw tiles from the first F frames only
        // (this kernel's own table: through ring_gather its forward launches ran 1.0-1.7 % slower: profiles/conv_ring_refactor.txt)
        const bool reflect = p.pad_mode == C2S_PAD_REFLECT;
#pragma unroll
        for (int i = 0; i < G::MAXE; ++i) {              // LDS float e = tid + 512 i of the raw tile: (channel, row, col)
            const int e = tid + i * 512;
            const int c = e / G::XP, rem = e - c * G::XP;
            int gy = oy0 - 1 + rem / G::RC, gx = ox0 - 1 + rem % G::RC;
            if (C2S_W16_DIAG == 13) gx += 1;
            if (C2S_W16_DIAG == 14) gx = ox0 + (rem % G::RC < 32 ? rem % G::RC : 31);
            if (C2S_W16_DIAG == 15 && gx < ox0) gx = ox0;                                  // no left halo column
            if (C2S_W16_DIAG == 16 && gx >= ox0 + 2 * BC) gx = ox0 + 2 * BC - 1;             // no right halo column
            if (C2S_W16_DIAG == 17) { if (gx < ox0) gx = ox0; if (gx >= ox0 + 2 * BC) gx = ox0 + 2 * BC - 1; }     // neither
            const bool ok = rem < G::PLANE && c < W16_CK &&
                            (reflect ? (gy <= p.H && gx <= p.W) : (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W));
            gy = reflect_idx(gy, p.H);                    // (identity inside the plane)
            gx = reflect_idx(gx, p.W);
            goff[i] = ok ? ((c * HW + gy * p.W + gx) * 4) : RING_OOB;
        }
        const float* s0n = p.src0 + (size_t)n * p.C0 * HW;
        const float* s1n = p.src1 != nullptr ? p.src1 + (size_t)n * p.C1 * HW : nullptr;
        r0 = __builtin_amdgcn_make_buffer_rsrc((void*)s0n, 0, p.C0 * HW * 4, 0x00020000);
        r1 = __builtin_amdgcn_make_buffer_rsrc((void*)(s1n != nullptr ? s1n : s0n), 0, p.C1 * HW * 4, 0x00020000);
    };
    // Requests (ring_stage_u / ring_stage_raw: the raw tile comes from HBM and is requested THREE chunks ahead of the MFMAs --
    // tools/wino16_diag.py: with two, ~130 us of the 64->64 @128^2 launch were waits for it -- U (L2 hits) two ahead).
    // Diagnostic builds 2, 5-7, 11, 12: nothing is staged after the first two chunks; 8 / 9 stop ONE stream (round 4: they had
    // fallen under the same switch since round 3 and measured 'no staging' three times over -- likewise 10)
    constexpr bool diag_stage = C2S_W16_DIAG != 2 && (C2S_W16_DIAG < 5 || (C2S_W16_DIAG >= 8 && C2S_W16_DIAG <= 10) || C2S_W16_DIAG >= 100);
    auto stage_u = [&](int k, int h0) {
        if ((C2S_W16_DIAG == 9 || !diag_stage) && diag_staged >= 2) return;
        ring_stage_u<G>(lds, (const C2S_AS1 char*)p.upk + ((size_t)blockIdx.y * K + k) * (G::USLAB * 4), h0, w, tid);
    };
    auto stage_raw = [&](int k, int slot) {
        const bool staged = !((C2S_W16_DIAG == 8 || !diag_stage) && diag_staged >= 2);
        ++diag_staged;
        if (!staged) return;
        const int cb_ = k * W16_CK;
        const bool first = cb_ < p.C0;
        const int chan0 = (first ? cb_ : cb_ - p.C0) * HW * 4;            // scalar offset of the request
        if (first) ring_stage_raw<G>(lds, r0, goff, chan0, slot, w);
        else ring_stage_raw<G>(lds, r1, goff, chan0, slot, w);
    };
    int tile = walk.first();
    if (tile >= walk.ntotal) return;
    RingCursor<true> cur = {tile};
    begin_staging(tile);
    auto request = [&](int h0, int slot) { cur.request(walk, K, h0, slot, begin_staging, stage_u, stage_raw); };
    int u0 = 0, rc = 0;                                // ring positions of the chunk being multiplied: U half slab of k-step 0, raw slot
    request(0, 0);
    request(0, 1);
    request(2, 2);

    // LDS offsets of this lane's operands inside a buffer
    const int aoff = kq * (4 * 64 * 4) + (32 * ch + t) * 4;                     // in a half slab [c 4][xi 4][o 64][nu 4]; + mt * 64 + xi * 256
    const int boff = G::URING + kq * G::XP + (2 * brow) * G::RC + 2 * (bcol0 + t);        // in a raw slot; + s * 4 * XP + r * RC
    auto load_a = [&](const float* ab, int mt, float (&a)[16]) {                 // ab: this lane's row of a half slab
        if (((C2S_W16_DIAG >= 4 && C2S_W16_DIAG <= 7) || C2S_W16_BARE) && ab != lds + aoff) return;
        ring_load_a<4, 256>(ab + mt * 64, a);          // one read per row xi (16 lanes: 256 contiguous bytes)
    };
    int boff0 = boff, boff1 = boff + 4 * G::XP;        // (the two k-steps)
    ring_opaque(boff0, boff1);
    auto load_d = [&](const float* bufp, int s, f32x2 (&dl)[4], f32x2 (&dh)[4]) {     // patch rows as (cols 0,1), (cols 2,3)
        if (((C2S_W16_DIAG >= 4 && C2S_W16_DIAG <= 7) || C2S_W16_BARE) && bufp != lds) return;
        ring_load_d<4, G::RC>(bufp + (s ? boff1 : boff0), dl, dh);
    };
    // adjoint folds of this wave's block row (scalar) and of this lane's block column
    float mtop = 0.f, mbot = 0.f;
    f32x2 mright = {0.f, 0.f}, mleft = {0.f, 0.f};     // (right, 0) and (0, left)
    bool rowfold = false, colfold = false;
    // V = Bt d B of one patch in 16 packed adds: rows on the column pairs, then per row xi (v0, v3) = L - H and
    // (v1, v2) = (L.y + H.x, H.x - L.y) (one VOP3P with operand selects); the s_nop covers the VALU -> MFMA wait states,
    // which the compiler cannot see through the asm
    auto transform = [&](const f32x2 (&dl_)[4], const f32x2 (&dh_)[4], float (&V)[16]) {
        f32x2 dl[4], dh[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { dl[r] = dl_[r]; dh[r] = dh_[r]; }
        if constexpr (ADJ) {
            if (rowfold) {
                dl[3] += mtop * dl[1]; dh[3] += mtop * dh[1];
                dl[0] += mbot * dl[2]; dh[0] += mbot * dh[2];
            }
            if (colfold) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x2 lo = dl[r], hi = dh[r];
                    dl[r] = lo + __builtin_shufflevector(hi, hi, 0, 0) * mright;     // col0 += right * col2
                    dh[r] = hi + __builtin_shufflevector(lo, lo, 1, 1) * mleft;      // col3 += left * col1
                }
            }
        }
        // (one asm block: left to itself the compiler unpacks part of this into scalar adds, and every VALU instruction costs
        // MFMA issue time; tl/th are scratch)
        f32x2 p03[4], p12[4], tl[4], th[4];
        asm("v_pk_add_f32 %8, %16, %18 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %9, %17, %18\n\t"
            "v_pk_add_f32 %10, %18, %17 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %11, %17, %19 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %12, %20, %22 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %13, %21, %22\n\t"
            "v_pk_add_f32 %14, %22, %21 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %15, %21, %23 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %0, %8, %12 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %4, %8, %12 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[1,0]\n\t"
            "v_pk_add_f32 %1, %9, %13 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %5, %9, %13 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[1,0]\n\t"
            "v_pk_add_f32 %2, %10, %14 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %6, %10, %14 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[1,0]\n\t"
            "v_pk_add_f32 %3, %11, %15 neg_lo:[0,1] neg_hi:[0,1]\n\t"
            "v_pk_add_f32 %7, %11, %15 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[1,0]\n\t"
            "s_nop 1"
            : "=&v"(p03[0]), "=&v"(p03[1]), "=&v"(p03[2]), "=&v"(p03[3]), "=&v"(p12[0]), "=&v"(p12[1]), "=&v"(p12[2]), "=&v"(p12[3]),
              "=&v"(tl[0]), "=&v"(tl[1]), "=&v"(tl[2]), "=&v"(tl[3]), "=&v"(th[0]), "=&v"(th[1]), "=&v"(th[2]), "=&v"(th[3])
            : "v"(dl[0]), "v"(dl[1]), "v"(dl[2]), "v"(dl[3]), "v"(dh[0]), "v"(dh[1]), "v"(dh[2]), "v"(dh[3]));
#pragma unroll
        for (int xi = 0; xi < 4; ++xi) {
            V[4 * xi] = p03[xi][0]; V[4 * xi + 1] = p12[xi][0]; V[4 * xi + 2] = p12[xi][1]; V[4 * xi + 3] = p03[xi][1];
        }
    };
    f32x4 acc[16][2];
    float* lbias = lds + G::BIAS;                      // the 64 channels' bias (behind the rings)
    // first = the first k-step of a tile: the accumulators start at 0 (an inline constant: no 128 v_mov per tile), those of
    // point (1,1) at the bias: At e11 A = [[1,1],[1,1]]
    auto mma = [&](const float (&a)[16], const float (&V)[16], int mt, bool first) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
#if C2S_W16_DIAG == 1
            asm volatile("" ::"v"(a[q]), "v"(V[q]));
#else
            if (first) {
                const f32x4 c0 = q == 5 ? *reinterpret_cast<const f32x4*>(lbias + 32 * ch + 16 * mt + 4 * kq) : (f32x4){0.f, 0.f, 0.f, 0.f};
                acc[q][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], V[q], c0, 0, 0, 0);
            } else {
                acc[q][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], V[q], acc[q][mt], 0, 0, 0);
            }
#endif
        }
    };

    // Schedule of one chunk: four half-steps (k-step s, channel group mt) of 16 MFMAs; the LDS reads of a half-step are issued
    // one half-step ahead (sched_barrier keeps the compiler from sinking them back to their use):
    //   (0,0) (0,1) | barrier (everyone's LDS-DMA of the NEXT chunk has landed: issued one chunk ago; everyone has left the
    //   PREVIOUS chunk's buffer) | request the chunk after next into that buffer | (1,0) | first reads of the next chunk | (1,1)
    float a0[16], a1[16], V[16];
    f32x2 dl[4], dh[4], el[4], eh[4];
    const int cof = co0 + 32 * ch + 4 * kq;            // this lane's output channels: cof + 16 mt + r (D rows 4 kq + r)
    if (tid < 64) lbias[tid] = (p.bias != nullptr && co0 + tid < p.Cout) ? p.bias[co0 + tid] : 0.f;
    __syncthreads();                                  // (drains the first requests: vmcnt(0))
    load_a(lds + aoff, 0, a0);
    load_d(lds, 0, dl, dh);
    while (true) {
        int n, oy0, ox0;
        walk.origin<2 * BR, 2 * BC>(tile, n, oy0, ox0);
        if constexpr (ADJ) {
            const int gbx = (ox0 >> 1) + bcol0 + t, gby = (oy0 >> 1) + brow, lastx = (p.W >> 1) - 1, lasty = (p.H >> 1) - 1;
            mleft = (f32x2){0.f, gbx == 0 ? 1.f : 0.f};
            mright = (f32x2){gbx == lastx ? 1.f : 0.f, 0.f};
            mtop = gby == 0 ? 1.f : 0.f;
            mbot = gby == lasty ? 1.f : 0.f;
            rowfold = gby == 0 || gby == lasty;
            colfold = ox0 == 0 || (ox0 >> 1) + BC > lastx;
        }
        auto chunk = [&](bool first) {
            const int u1 = u0 == 4 ? 0 : u0 + 1, u2 = u1 == 4 ? 0 : u1 + 1;    // this chunk's second half slab; the next chunk's first
            const float* xb = lds + rc * G::XS;
            load_a(lds + u0 * G::UHALF + aoff, 1, a1);
            __builtin_amdgcn_sched_barrier(0);
            if ((C2S_W16_DIAG != 7 && !C2S_W16_BARE) || first) transform(dl, dh, V);
            __builtin_amdgcn_sched_barrier(0);
            load_d(xb, 1, el, eh);                     // (after the transform: its temporaries are dead)
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, V, 0, first);
            __builtin_amdgcn_sched_barrier(0);
            load_a(lds + u1 * G::UHALF + aoff, 0, a0);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, V, 1, first);
            __builtin_amdgcn_sched_barrier(0);
            // everyone's requests for the NEXT chunk have landed (U: issued one chunk ago; raw: two); the six youngest (the
            // raw pieces of the chunk after next) may stay in flight -- loads complete in order
#ifdef C2S_W16_STAMP
            const unsigned long long st_t0 = __builtin_amdgcn_s_memtime();
#endif
            if (C2S_W16_DIAG != 6 && C2S_W16_DIAG != 12) ring_wait_landed<G>(cur.young_raw);
#ifdef C2S_W16_STAMP
            st_wait += __builtin_amdgcn_s_memtime() - st_t0;
            if (first) st_first += __builtin_amdgcn_s_memtime() - st_t0;
            ++st_chunks;
#endif
            __builtin_amdgcn_sched_barrier(0);
            request(u0 == 0 ? 4 : u0 - 1, (rc + 3) & 3);       // U of the chunk after next: half slabs u0 + 4, u0 + 5 = u0 (mod 5)
            load_a(lds + u1 * G::UHALF + aoff, 1, a1);
            __builtin_amdgcn_sched_barrier(0);
            if (C2S_W16_DIAG != 7 && !C2S_W16_BARE) transform(el, eh, V);
            mma(a0, V, 0, false);
            __builtin_amdgcn_sched_barrier(0);
            load_a(lds + u2 * G::UHALF + aoff, 0, a0);                  // (after the last chunk of the last tile: stale, unused)
            load_d(lds + ((rc + 1) & 3) * G::XS, 0, dl, dh);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, V, 1, false);
            __builtin_amdgcn_sched_barrier(0);
            u0 = u2;
            rc = (rc + 1) & 3;
        };
        chunk(true);
        for (int k = 1; k < K; ++k) chunk(false);
#ifdef C2S_W16_STAMP
        const unsigned long long st_e0 = __builtin_amdgcn_s_memtime();
#endif
        asm volatile("s_nop 7\n\ts_nop 7");             // the last MFMA results are readable by the asm adds of the epilogue
        __builtin_amdgcn_sched_barrier(0);
        // ---- epilogue: At M A per (channel, block) in registers, on channel PAIRS (the accumulator's adjacent registers:
        // v_pk_add_f32), transposed to (column 0, column 1) for one 8-byte store per output row; lane (t, kq): channels
        // cof + 16 mt + r, block (brow, t).  Buffer stores: the channel offset is scalar, an out-of-plane lane or a padded
        // channel is an out-of-range offset -- no address arithmetic or lane masks in the vector ALU
        const int oy = oy0 + 2 * brow, ox = ox0 + 2 * (bcol0 + t);
        const __amdgpu_buffer_rsrc_t ro =
            __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + (size_t)n * p.Cout * HW), 0, p.Cout * HW * 4, 0x00020000);
        const bool in0 = ox < p.W && oy < p.H && C2S_W16_DIAG != 3, in1 = in0 && oy + 1 < p.H;
#if C2S_W16_BARE
        {   // no output transform, no stores: one dependent use keeps the accumulators alive
            float keepalive = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) keepalive += acc[q][0][0] + acc[q][1][0];
            if (keepalive == 12345.678f) p.out[0] = keepalive;
        }
        if (cur.stile >= walk.ntotal) break;
        tile = cur.stile;
        continue;
#endif
        const int vo0 = in0 ? (cof * HW + oy * p.W + ox) * 4 : RING_OOB;
        const int vo1 = in1 ? vo0 + p.W * 4 : RING_OOB;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 P0[4], P1[4];
#pragma unroll
                for (int xi = 0; xi < 4; ++xi) {
                    f32x2 m[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) m[j] = (f32x2){acc[4 * xi + j][mt][2 * h], acc[4 * xi + j][mt][2 * h + 1]};
                    P0[xi] = m[0] + m[1] + m[2];
                    P1[xi] = sub2(m[1], m[2], m[3]);
                }
                const f32x2 Y00 = P0[0] + P0[1] + P0[2], Y01 = P1[0] + P1[1] + P1[2];
                const f32x2 Y10 = sub2(P0[1], P0[2], P0[3]), Y11 = sub2(P1[1], P1[2], P1[3]);
                f32x2 y[2][2] = {{(f32x2){Y00[0], Y01[0]}, (f32x2){Y10[0], Y11[0]}},        // [channel of the pair][output row]
                                 {(f32x2){Y00[1], Y01[1]}, (f32x2){Y10[1], Y11[1]}}};
                ring_store_rows(ro, vo0, vo1, (16 * mt + 2 * h) * HW * 4, HW * 4, p.accumulate, y);
            }
        }
#ifdef C2S_W16_STAMP
        st_epi += __builtin_amdgcn_s_memtime() - st_e0;
#endif
        if (cur.stile >= walk.ntotal) break;
        tile = cur.stile;
    }
#ifdef C2S_W16_STAMP
    if (tid == 0 && blockIdx.x < 1024 && blockIdx.y == 0) {
        w16_stamps[blockIdx.x * 4 + 0] = st_wait;
        w16_stamps[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memtime() - st_begin;
        w16_stamps[blockIdx.x * 4 + 2] = st_chunks | (st_first << 20);
        w16_stamps[blockIdx.x * 4 + 3] = st_epi;
    }
#endif
}

void init_hook() {
    C2S_RAISE_LDS((conv_winograd16_kernel<false, 4, 16>));
    C2S_RAISE_LDS((conv_winograd16_kernel<true, 4, 16>));
}
C2sInitRegistrar registrar(init_hook);

}  // namespace

#ifdef C2S_W16_STAMP
extern "C" int c2s_debug_w16_stamps(unsigned long long* host_out) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(w16_stamps), sizeof(unsigned long long) * 1024 * 4) == hipSuccess ? 0 : 1;
}
#endif

extern "C" int c2s_conv3x3_winograd16_supported(const c2s_conv_desc* d) {
    return d && d->KH == 3 && d->KW == 3 && d->S == 1 && d->pad_y == 1 && d->pad_x == 1 && d->Hin % 2 == 0 && d->Win % 2 == 0 &&
           d->Win >= 32 && d->Hin >= 8 && d->CoutP % 64 == 0 && d->C0 + d->C1 > 3 * W16_CK && d->C0 % W16_CK == 0 &&
           d->C1 % W16_CK == 0 && d->N <= ring_max_frames<W16Shape<4, 16>::G>();
                                                   // whole chunks only: the chunk's channel base travels in the SGPR offset of the
                                                   // LDS-DMA loads, which takes no part in the buffer range check -- a ragged
                                                   // last chunk would read the next frame (ragged counts: the 4-wave kernel)
}

extern "C" int c2s_conv3x3_winograd16(const c2s_conv_desc* d, const float* src0, const float* src1, const float* upk,
                                      const float* bias, float* out, const int* valid, void* stream) {
    // tile shape: 4 x 16 blocks = 8 x 32 output pixels (the kernel is a template on it; 2 x 32 blocks = 4 x 64 pixels, with one
    // 66-float raw row per request instead of two of 34, measured 696 / 755 us against 684 / 742 on the 64 -> 64 @128^2 layer)
    constexpr int BRh = 4, BCh = 16;
    using G = W16Shape<BRh, BCh>::G;
    if (int rc = ring_check("conv3x3_winograd16", d, src0 && upk && out, ring_max_frames<G>(), 1L << 31, true)) return rc;
    C2S_REQUIRE(c2s_conv3x3_winograd16_supported(d), "conv3x3_winograd16: 3x3 stride 1 pad 1, even planes at least 32 wide and 8 high, CoutP %% 64, channels of each source a multiple of 8");
    C2S_REQUIRE(d->C0 > 0 && d->C1 >= 0 && (d->C1 == 0 || src1), "conv3x3_winograd16: bad channels");
    C2S_REQUIRE(d->Hout == d->Hin && d->Wout == d->Win, "conv3x3_winograd16: same-size output only");
    C2S_REQUIRE(d->CoutP >= d->Cout && d->Cout > 0, "conv3x3_winograd16: bad CoutP");
    if (d->reflect_adjoint) C2S_REQUIRE(d->pad_mode == C2S_PAD_ZEROS, "conv3x3_winograd16: the reflect adjoint is a zero-padded launch");
    Wino16Params p;
    p.src0 = src0; p.src1 = src1; p.upk = upk; p.bias = bias; p.out = out; p.valid = valid;
    p.C0 = d->C0; p.C1 = d->C1; p.H = d->Hin; p.W = d->Win; p.Cout = d->Cout; p.CoutP = d->CoutP;
    p.pad_mode = d->pad_mode; p.accumulate = d->accumulate;
    p.tiles_x = cdiv(d->Win, 2 * BCh);
    p.tiles = p.tiles_x * cdiv(d->Hin, 2 * BRh);
    p.N = d->N;
    p.nchunks = cdiv(d->C0 + d->C1, W16_CK);
    const dim3 grid = ring_grid(d->CoutP / 64, (long)d->N * p.tiles, 1);
    const size_t ldsb = ring_lds_bytes<G>(d->N);
    hipStream_t st = (hipStream_t)stream;
    if (d->reflect_adjoint) hipLaunchKernelGGL((conv_winograd16_kernel<true, BRh, BCh>), grid, dim3(512), ldsb, st, p);
    else hipLaunchKernelGGL((conv_winograd16_kernel<false, BRh, BCh>), grid, dim3(512), ldsb, st, p);
    C2S_CHECK_LAUNCH("conv3x3_winograd16");
    return C2S_OK;
}
