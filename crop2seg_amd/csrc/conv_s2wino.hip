// 4x4 stride-2 pad-1 convolution (forward) as Winograd F(2x2, 2x2) over the four input parities, on the structure of
// conv_winograd16.hip (8 waves, v_mfma_f32_16x16x4_f32, all transform points of a (channel, block) in one lane, operands by
// LDS-DMA into rings, requests two / three chunks ahead of the MFMAs).
//
// With x0[i] = x[2i], x1[i] = x[2i+1] (the two parities of a row) the 4-tap stride-2 filter is two 2-tap stride-1 filters with
// shifted windows:   y[i] = x1[i-1] w0 + x0[i] w1 + x1[i] w2 + x0[i+1] w3
//   parity 0: window (x0[i], x0[i+1]),   taps (w1, w3);      parity 1: window (x1[i-1], x1[i]),   taps (w0, w2)
// so a 2x2 output block needs a 3x3 patch of each of the four (row parity, column parity) planes, and F(2x2, 2x2)
//   Y = At [ sum_{c, parity} (G g Gt) (.) (Bt d B) ] A,   Bt = [[1,-1,0],[0,1,0],[0,-1,1]],  G = [[1,0],[1,1],[0,1]],  At = [[1,1,0],[0,1,1]]
// takes 9 multiplies per (input channel, parity) and block instead of 16: 36 instead of 64 per (cin, cout) pair and 2x2 block.
// The transform matrices are integer: the arithmetic is as exact as the direct form's.
// MFMA mapping: k index of the 16x16x4 MFMA = the parity (one k-step = one input channel), lane (t = block column, kq = parity)
// transforms the 3x3 patch of its parity plane; A operand = U[p][(c, parity)][o], 9 points padded to 12 floats (three
// conflict-free ds_read_b128).  A chunk is two input channels: 24 KB of U (two half slabs of a ring of five) and the eight
// parity planes of the 8 x 32 output tile (9 x 33 each, gathered by buffer_load_dword ... lds with reflected / stride-2 source
// addresses; ring of four).  Wave w: output channels 32 (w & 1) .., block rows 2 (w >> 1), 2 (w >> 1) + 1 (an A operand
// serves two block rows: half the U traffic per MFMA of a one-row wave); accumulators acc[9][2][2] of 16x16.
//
// Reference call sites replaced: nn.Conv2d(4, stride 2, padding 1, reflect) of DownConvBlock (src/backbones/conv.py:263-271)
// for layers with an even number (>= 8) of input channels on output planes at least 32 wide (the engine keeps
// conv_igemm_kernel<4,2,*> for the rest; C2S_S2WINO=0 keeps it everywhere).
#include "conv_ring.h"
#include <stdlib.h>

namespace {

struct S2wParams {
    const float* src;
    const float* upk;      // [cout block][chunk][2 c][4 parities][64 o][12] (9 points + 3 pad)
    const float* bias;
    float* out;
    const int* valid;
    int Cin, Hin, Win, H, W, Cout, CoutP;     // H, W: the output plane
    int pad_mode, accumulate;
    int N, tiles, tiles_x, nchunks;
};

constexpr int S2_BR = 8, S2_BC = 16;                 // blocks per tile: 8 rows x 16 columns = 16 x 32 output pixels
// a k-step = one input channel, four parities: 3,072 floats = 12 KB of U; a chunk of two channels: 24 KB, three 16-byte pieces per
// thread; raw ring of four slots of the chunk's eight parity planes (17 rows x 33 columns, row pitch 34); the bias of 64 channels
using S2G = RingGeom<4 * 64 * S2_UP, 4, 8, 2 * S2_BR + 1, 34, 608, 64>;

__global__ __launch_bounds__(512, 1) void conv_s2wino_kernel(S2wParams p) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & 15, kq = lane >> 4;        // block column / parity (B, D: channel quad) ; A: output channel / parity
    const int ch = w & 1, brow = w >> 1;            // channel half (32) and block row of this wave
    const int co0 = blockIdx.y * 64;
    const int HWin = p.Hin * p.Win, HWo = p.H * p.W;
    const int K = p.nchunks;

    const RingWalk walk = {reinterpret_cast<unsigned*>(lds + S2G::FLAGS), p.N * p.tiles, p.tiles, p.tiles_x};
    ring_frame_flags(reinterpret_cast<unsigned*>(lds + S2G::FLAGS), p.valid, p.N, tid);
    float* lbias = lds + S2G::BIAS;
    if (tid < 64) lbias[tid] = (p.bias != nullptr && co0 + tid < p.Cout) ? p.bias[co0 + tid] : 0.f;
    __syncthreads();

    // ---- the staging side (its own tile state): plane pc = 4 c + parity of the chunk, parity = 2 py + px; plane element
    // (r, q) is the input pixel (2 (oy0 + r) - py, 2 (ox0 + q) - px); the pitch's 34th column is not used
    int goff[S2G::MAXE];
    __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, 0, 0x00020000);
    auto begin_staging = [&](int tt) __attribute__((always_inline)) {
        int n, oy0, ox0;
        walk.origin<2 * S2_BR, 2 * S2_BC>(tt, n, oy0, ox0);
        ring_gather<S2G>(goff, tid, p.Hin, p.Win, p.pad_mode, [&](int pc, int r, int q, int& c, int& gy, int& gx) {
            c = pc >> 2;
            gy = 2 * (oy0 + r) - ((pc >> 1) & 1); gx = 2 * (ox0 + q) - (pc & 1);
            return q < 2 * S2_BC + 1;
        });
        r0 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.src + (size_t)n * p.Cin * HWin), 0, p.Cin * HWin * 4, 0x00020000);
    };
    auto stage_u = [&](int k, int h0) __attribute__((always_inline)) {
        ring_stage_u<S2G>(lds, (const C2S_AS1 char*)p.upk + ((size_t)blockIdx.y * K + k) * (S2G::USLAB * 4), h0, w, tid);
    };
    auto stage_raw = [&](int k, int slot) __attribute__((always_inline)) {
        ring_stage_raw<S2G>(lds, r0, goff, 2 * k * HWin * 4, slot, w);
    };
    int tile = walk.first();
    if (tile >= walk.ntotal) return;
    RingCursor<true> cur = {tile};                     // raw planes three chunks ahead, U two ahead
    begin_staging(tile);
    auto request = [&](int h0, int slot) __attribute__((always_inline)) { cur.request(walk, K, h0, slot, begin_staging, stage_u, stage_raw); };
    int u0 = 0, rc = 0;                                // ring positions of the chunk being multiplied
    request(0, 0);
    request(0, 1);
    request(2, 2);

    // LDS offsets of this lane's operands
    const int aoff = (kq * 64 + 32 * ch + t) * S2_UP;                          // in a half slab; + mt * 16 * UP
    const int boff = S2G::URING + kq * S2G::XP + (4 * brow) * S2G::RC + 2 * t;  // in a raw slot (block row 2 brow); + s * 4 * XP + (2 br + r) * RC
    auto load_a = [&](const float* ab, int mt, float (&a)[12]) { ring_load_a<3, 4>(ab + mt * 16 * S2_UP, a); };     // (9 used)
    int boff0 = boff, boff1 = boff + 4 * S2G::XP;      // (the two k-steps)
    ring_opaque(boff0, boff1);
    // the patches of the wave's two block rows share their middle row: five rows
    auto load_d = [&](const float* bufp, int s, f32x2 (&dl)[5], f32x2 (&dh)[5]) { ring_load_d<5, S2G::RC>(bufp + (s ? boff1 : boff0), dl, dh); };
    // V = Bt d B of the 3x3 patch (point p = 3 xi + nu)
    auto transform = [&](f32x2 l0, f32x2 l1, f32x2 l2, f32x2 h0, f32x2 h1, f32x2 h2, float (&V)[9]) {
        const f32x2 tl[3] = {l0 - l1, l1, l2 - l1};
        const float th[3] = {h0[0] - h1[0], h1[0], h2[0] - h1[0]};
#pragma unroll
        for (int xi = 0; xi < 3; ++xi) {
            V[3 * xi] = tl[xi][0] - tl[xi][1];
            V[3 * xi + 1] = tl[xi][1];
            V[3 * xi + 2] = th[xi] - tl[xi][1];
        }
    };
    f32x4 acc[9][2][2];                                // [point][channel group][block row]
    // first = the first k-step of a tile: accumulators start at 0 (inline constant), those of point (1,1) at the bias
    // (At e11 A = [[1,1],[1,1]])
    auto mma = [&](const float (&a)[12], const float (&V)[9], int mt, int br, bool first) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            if (first) {
                const f32x4 c0 = q == 4 ? *reinterpret_cast<const f32x4*>(lbias + 32 * ch + 16 * mt + 4 * kq) : (f32x4){0.f, 0.f, 0.f, 0.f};
                acc[q][mt][br] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], V[q], c0, 0, 0, 0);
            } else {
                acc[q][mt][br] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], V[q], acc[q][mt][br], 0, 0, 0);
            }
        }
    };

    float a0[12], a1[12], V0[9], V1[9];
    f32x2 dl[5], dh[5];
    const int cof = co0 + 32 * ch + 4 * kq;            // this lane's output channels: cof + 16 mt + r (D rows 4 kq + r)
    __syncthreads();                                  // (drains the first requests: vmcnt(0))
    load_a(lds + aoff, 0, a0);
    load_d(lds, 0, dl, dh);
    while (true) {
        int n, oy0, ox0;
        walk.origin<2 * S2_BR, 2 * S2_BC>(tile, n, oy0, ox0);
        // one k-step (one input channel): four half-steps (channel group, block row) of 9 MFMAs; the A operand of a channel
        // group is read one group ahead; the next k-step's patch rows are read once both transforms have consumed the current
        auto kstep = [&](const float* A, const float* Anext, const float* Xnext, int snext, bool first) __attribute__((always_inline)) {
            load_a(A, 1, a1);
            __builtin_amdgcn_sched_barrier(0);
            transform(dl[0], dl[1], dl[2], dh[0], dh[1], dh[2], V0);
            transform(dl[2], dl[3], dl[4], dh[2], dh[3], dh[4], V1);
            __builtin_amdgcn_sched_barrier(0);
            load_d(Xnext, snext, dl, dh);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, V0, 0, 0, first);
            mma(a0, V1, 0, 1, first);
            __builtin_amdgcn_sched_barrier(0);
            load_a(Anext, 0, a0);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, V0, 1, 0, first);
            mma(a1, V1, 1, 1, first);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto chunk = [&](bool first) __attribute__((always_inline)) {
            const int u1 = u0 == 4 ? 0 : u0 + 1, u2 = u1 == 4 ? 0 : u1 + 1;
            kstep(lds + u0 * S2G::UHALF + aoff, lds + u1 * S2G::UHALF + aoff, lds + rc * S2G::XS, 1, first);
            ring_wait_landed<S2G>(cur.young_raw);
            __builtin_amdgcn_sched_barrier(0);
            request(u0 == 0 ? 4 : u0 - 1, (rc + 3) & 3);       // chunk after next: half slabs u0 + 4, u0 (mod 5); raw of the one after
            // (after the last chunk of the last tile the tail reads are stale and unused)
            kstep(lds + u1 * S2G::UHALF + aoff, lds + u2 * S2G::UHALF + aoff, lds + ((rc + 1) & 3) * S2G::XS, 0, false);
            u0 = u2;
            rc = (rc + 1) & 3;
        };
        chunk(true);
        for (int k = 1; k < K; ++k) chunk(false);
        // ---- epilogue: At M A on channel pairs; P[xi][0] = M[xi][0] + M[xi][1], P[xi][1] = M[xi][1] + M[xi][2];
        // Y[0][j] = P[0][j] + P[1][j], Y[1][j] = P[1][j] + P[2][j]; buffer stores (ring_store_rows)
        const int ox = ox0 + 2 * t;
        const __amdgpu_buffer_rsrc_t ro =
            __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + (size_t)n * p.Cout * HWo), 0, p.Cout * HWo * 4, 0x00020000);
#pragma unroll
        for (int br = 0; br < 2; ++br) {
        const int oy = oy0 + 2 * (2 * brow + br);
        const bool in0 = ox < p.W && oy < p.H, in1 = in0 && oy + 1 < p.H;
        const int vo0 = in0 ? (cof * HWo + oy * p.W + ox) * 4 : RING_OOB;
        const int vo1 = in1 ? vo0 + p.W * 4 : RING_OOB;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 P0[3], P1[3];
#pragma unroll
                for (int xi = 0; xi < 3; ++xi) {
                    f32x2 m[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) m[j] = (f32x2){acc[3 * xi + j][mt][br][2 * h], acc[3 * xi + j][mt][br][2 * h + 1]};
                    P0[xi] = m[0] + m[1];
                    P1[xi] = m[1] + m[2];
                }
                const f32x2 Y00 = P0[0] + P0[1], Y01 = P1[0] + P1[1], Y10 = P0[1] + P0[2], Y11 = P1[1] + P1[2];
                f32x2 y[2][2] = {{(f32x2){Y00[0], Y01[0]}, (f32x2){Y10[0], Y11[0]}},        // [channel of the pair][output row]
                                 {(f32x2){Y00[1], Y01[1]}, (f32x2){Y10[1], Y11[1]}}};
                ring_store_rows(ro, vo0, vo1, (16 * mt + 2 * h) * HWo * 4, HWo * 4, p.accumulate, y);
            }
        }
        }
        if (cur.stile >= walk.ntotal) break;
        tile = cur.stile;
    }
}

void init_hook() {
    C2S_RAISE_LDS(conv_s2wino_kernel);
}
C2sInitRegistrar registrar(init_hook);

}  // namespace

extern "C" int c2s_conv4x4s2_winograd_supported(const c2s_conv_desc* d) {
    return d && d->KH == 4 && d->KW == 4 && d->S == 2 && d->pad_y == 1 && d->pad_x == 1 && d->C1 == 0 && d->C0 % 2 == 0 &&
           d->C0 >= 8 && d->Hin == 2 * d->Hout && d->Win == 2 * d->Wout && d->Hout % 2 == 0 && d->Wout % 2 == 0 &&
           d->Wout >= 32 && d->Hout >= 8 && d->CoutP % 64 == 0 && d->reflect_adjoint == 0 && d->N <= ring_max_frames<S2G>();
}

extern "C" int c2s_conv4x4s2_winograd(const c2s_conv_desc* d, const float* src, const float* upk, const float* bias,
                                      float* out, const int* valid, void* stream) {
    if (int rc = ring_check("conv4x4s2_winograd", d, src && upk && out, ring_max_frames<S2G>(), RING_OOB, true)) return rc;
    C2S_REQUIRE(c2s_conv4x4s2_winograd_supported(d), "conv4x4s2_winograd: 4x4 stride 2 pad 1, one source with an even number (>= 8) of channels, even output planes at least 32 wide and 8 high, CoutP %% 64");
    C2S_REQUIRE(d->Cout > 0 && d->CoutP >= d->Cout, "conv4x4s2_winograd: bad Cout");
    S2wParams p;
    p.src = src; p.upk = upk; p.bias = bias; p.out = out; p.valid = valid;
    p.Cin = d->C0; p.Hin = d->Hin; p.Win = d->Win; p.H = d->Hout; p.W = d->Wout; p.Cout = d->Cout; p.CoutP = d->CoutP;
    p.pad_mode = d->pad_mode; p.accumulate = d->accumulate;
    p.tiles_x = cdiv(d->Wout, 2 * S2_BC);
    p.tiles = p.tiles_x * cdiv(d->Hout, 2 * S2_BR);
    p.N = d->N;
    p.nchunks = d->C0 / 2;
    const dim3 grid = ring_grid(d->CoutP / 64, (long)d->N * p.tiles, 1);
    hipLaunchKernelGGL(conv_s2wino_kernel, grid, dim3(512), ring_lds_bytes<S2G>(d->N), (hipStream_t)stream, p);
    C2S_CHECK_LAUNCH("conv4x4s2_winograd");
    return C2S_OK;
}
