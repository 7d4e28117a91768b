// Data gradient of the 4x4 stride-2 pad-1 convolution (= a transposed convolution) as Winograd F(2x2, 2x2) per output parity,
// on the structure of conv_s2wino.hip / conv_winograd16.hip.
//
// With u = 2m + e (e = parity of the input-resolution row u) the gradient is a 2-tap stride-1 filter over gy per parity:
//   gx[2m]   = gy[m-1] w3 + gy[m] w1        (e = 0: window gy[m-1 .. ], taps (w3, w1))
//   gx[2m+1] = gy[m]   w2 + gy[m+1] w0      (e = 1: window gy[m   .. ], taps (w2, w0))
// so a pair of outputs (m, m+1) of one parity needs three gy values and F(2,2) takes 3 multiplies instead of 4 per dimension:
// 9 instead of 16 per (gy channel, parity, 2x2 block of the parity plane).  A workgroup takes ONE row parity ey (grid.y), its
// lanes BOTH column parities ex: the two 3-wide column windows of a block overlap in two columns (one 4-float read), and the
// four outputs (n, ex) of a row are contiguous in gx: one 16-byte store.  The MFMA's output rows are the "virtual channels"
// (ex, cin): a wave owns 32 input channels x 2 column parities x 16 blocks = acc[9][2][2] of 16x16.
//
// Reflect padding of the forward pass: the gradient of the halo rows/columns (u = -1 and u = 2 Ho) is added to u = 1 and
// u = 2 Ho - 2.  The halo term of u = 1 is gy[0] w0 = g1 d0 of the first block of parity 1 -- not expressible by changing the
// data of the standard F(2,2) points, but another 3-multiply algorithm computes both outputs INCLUDING it:
//   first output folds ("top"):   V = (d1, d0 + d1, d2),   y0 = -m0 + m1,  y1 = m0 + m2     (y0 = g0 d0 + g1 (d0 + d1))
//   last output folds ("bottom"): V = (d0, d1 + d2, d1),   y0 =  m0 + m2,  y1 = m1 - m2     (y1 = g0 (d1 + d2) + g1 d2)
// with the same weights U = (g0, g0 + g1, g1).  Rows: per wave (uniform branch); columns: per lane (0/1 masks), only in tiles
// that touch the left / right edge.  No border kernel, no second pass.
//
// Reference call site replaced: convolution_backward-input of nn.Conv2d(4, stride 2, padding 1, reflect) in DownConvBlock
// (src/backbones/conv.py:263-271), for layers with a multiple of 8 (>= 24) output channels on planes at least 32 wide
// (C2S_S2WINO=0 keeps conv_xpair_kernel).
#include "conv_ring.h"
#include <stdlib.h>

namespace {

struct S2dParams {
    const float* src;      // gy [N][Kc][Ho][Wo]
    const float* upk;      // [ey 2][cin block][chunk][2 k-steps][4 k][128 = ex * 64 + cin][12]
    float* out;            // gx [N][Cs][2 Ho][2 Wo]
    const int* valid;
    int Kc, Ho, Wo, Cs, CsP;
    int fold, accumulate;
    int N, tiles, tiles_x, nchunks;
    // SKIP: out = this gradient + round(a_up * gskip), the skip term of the temporal aggregation (aggregate.hip)
    // (read from the kernel arguments where the epilogue needs them, not held in SGPRs across the chunk loop)
    const float* a_up;     // [n_head][N][2 Ho][2 Wo], frame n = b T + t
    const float* gskip;    // [N / T][Cs][2 Ho][2 Wo]
    int T, cpg_log2, a_bytes;      // a_bytes: ((n_head - 1) N + 1) 4 Ho Wo * 4, the bytes of a_up a frame's resource spans
};

// a k-step = 4 gy channels x 128 virtual channels: a half slab of 6,144 floats = 24 KB of U; a chunk of 8 gy channels: 48 KB, six
// 16-byte pieces per thread; raw ring of three slots of the chunk's 8 channels (9 rows x 34 columns); no bias: 159,744 B (+ flags)
using D2G = RingGeom<4 * 128 * D2_UP, 3, 8, 9, 34, 352, 0>;

// a * b rounded on its own: what a kernel that stores the product and one that adds it to something must agree on
__device__ __forceinline__ f32x4 rounded_product(f32x4 a, f32x4 b) {
#pragma clang fp contract(off)
    return a * b;
}
#define C2S_AS4 __attribute__((address_space(4)))

template <bool SKIP>
__global__ __launch_bounds__(512, 1) void conv_s2dgrad_kernel(S2dParams p) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = lane & 15, kq = lane >> 4;        // block column / k index (B; D: channel quad) ; A: virtual channel / k index
    const int ch = w & 1, brow = w >> 1;            // input-channel half (32) and block row of this wave
    const int ey = blockIdx.y & 1, cblk = blockIdx.y >> 1;
    const int HWo = p.Ho * p.Wo, Hin = 2 * p.Ho, Win = 2 * p.Wo, HWin = Hin * Win;
    const int K = p.nchunks;

    const RingWalk walk = {reinterpret_cast<unsigned*>(lds + D2G::FLAGS), p.N * p.tiles, p.tiles, p.tiles_x};
    ring_frame_flags(reinterpret_cast<unsigned*>(lds + D2G::FLAGS), p.valid, p.N, tid);
    __syncthreads();

    // ---- staging side.  Tile (ty, tx): parity-plane rows 8 ty .. 8 ty + 7 (4 block rows), columns 32 tx .. 32 tx + 31 (16 block
    // columns); raw tile element (c, r, q) = gy[8 k + c][m0 - 1 + ey + r][n0 - 1 + q], zero outside the plane.  The gather table
    // and the U requests are this kernel's own text: through ring_gather / ring_stage_u (conv_ring.h) it came out with more
    // scratch and a spill inside the chunk loop (profiles/conv_ring_refactor.txt)
    int goff[D2G::MAXE];
    __amdgpu_buffer_rsrc_t r0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, 0, 0x00020000);
    auto begin_staging = [&](int tt) {
        int n, m0, n0;
        walk.origin<8, 32>(tt, n, m0, n0);
#pragma unroll
        for (int i = 0; i < D2G::MAXE; ++i) {
            const int e = tid + i * 512;
            const int c = e / D2G::XP, rem = e - c * D2G::XP;
            const int r = rem / D2G::RC, q = rem - r * D2G::RC;
            const int gy = m0 - 1 + ey + r, gx = n0 - 1 + q;
            const bool ok = rem < D2G::PLANE && c < 8 && gy >= 0 && gy < p.Ho && gx >= 0 && gx < p.Wo;
            goff[i] = ok ? ((c * HWo + gy * p.Wo + gx) * 4) : RING_OOB;
        }
        r0 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.src + (size_t)n * p.Kc * HWo), 0, p.Kc * HWo * 4, 0x00020000);
    };
    auto stage_u = [&](int k, int h0) {                // U chunk k (48 KB): three pieces per half slab h0, h0 + 1 (mod 5)
        const int h1 = h0 == 4 ? 0 : h0 + 1;
        const C2S_AS1 char* g = (const C2S_AS1 char*)p.upk + ((size_t)(ey * (p.CsP / 64) + cblk) * K + k) * (D2G::USLAB * 4);
        float* d0 = lds + h0 * D2G::UHALF + w * 256;
        float* d1 = lds + h1 * D2G::UHALF + w * 256;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            float* dst = (i < 3 ? d0 : d1) + (i % 3) * 2048;
            __builtin_amdgcn_global_load_lds((const C2S_AS1 void*)(g + i * 8192 + (unsigned)(tid * 16)), (C2S_AS3 void*)dst, 16, 0, 0);
        }
    };
    auto stage_raw = [&](int k, int slot) { ring_stage_raw<D2G>(lds, r0, goff, 8 * k * HWo * 4, slot, w); };
    int tile = walk.first();
    if (tile >= walk.ntotal) return;
    RingCursor<false> cur = {tile};                    // both operands two chunks ahead: one ring slot less than the forward kernels
    begin_staging(tile);
    auto request = [&](int h0, int slot) { cur.request(walk, K, h0, slot, begin_staging, stage_u, stage_raw); };
    int u0 = 0, rc = 0;                                // ring positions of the chunk being multiplied
    request(0, 0);
    request(2, 1);

    // LDS offsets of this lane's operands
    const int aoff = (kq * 128 + 32 * ch + t) * D2_UP;                          // in a half slab; + (ex * 64 + mt * 16) * UP
    const int boff = D2G::URING + kq * D2G::XP + (2 * brow) * D2G::RC + 2 * t;  // in a raw slot; + s * 4 * XP + r * RC
    auto load_a = [&](const float* ab, int ex, int mt, float (&a)[12]) { ring_load_a<3, 4>(ab + (ex * 64 + mt * 16) * D2_UP, a); };
    int boff0 = boff, boff1 = boff + 4 * D2G::XP;      // (the two k-steps)
    ring_opaque(boff0, boff1);
    auto load_d = [&](const float* bufp, int s, f32x2 (&dl)[3], f32x2 (&dh)[3]) { ring_load_d<3, D2G::RC>(bufp + (s ? boff1 : boff0), dl, dh); };
    // fold state of the tile being multiplied: rows per wave (rt: 0 standard, 1 first output folds, 2 last output folds),
    // columns per lane (fl: column parity 1 of block column 0; fr: column parity 0 of the last block column)
    int rt = 0;
    float fl = 0.f, fr = 0.f;
    bool colfold = false;
    // row stage of a patch (in place: rows become the three row points), then the column stage of one column parity:
    // V[3 xi + nu]
    auto transform_rows = [&](f32x2 (&dl)[3], f32x2 (&dh)[3]) {
        const f32x2 l0 = dl[0], l1 = dl[1], l2 = dl[2], h0 = dh[0], h1 = dh[1], h2 = dh[2];
        if (rt == 0) {
            dl[0] = l0 - l1; dl[2] = l2 - l1;
            dh[0] = h0 - h1; dh[2] = h2 - h1;
        } else if (rt == 1) {
            dl[0] = l1; dl[1] = l0 + l1;
            dh[0] = h1; dh[1] = h0 + h1;
        } else {
            dl[1] = l1 + l2; dl[2] = l1;
            dh[1] = h1 + h2; dh[2] = h1;
        }
    };
    auto transform_cols = [&](const f32x2 (&tl)[3], const f32x2 (&th)[3], int ex, float (&V)[9]) {
#pragma unroll
        for (int xi = 0; xi < 3; ++xi) {
            const float c0 = tl[xi][0], c1 = tl[xi][1], c2 = th[xi][0], c3 = th[xi][1];
            if (ex == 0) {                       // window (c0, c1, c2): the last output may fold (fr)
                float a0 = c0 - c1, a1 = c1, a2 = c2 - c1;
                if (colfold) { a0 = fmaf(fr, c1, a0); a1 = fmaf(fr, c2, a1); a2 = fmaf(fr, 2.f * c1 - c2, a2); }
                V[3 * xi] = a0; V[3 * xi + 1] = a1; V[3 * xi + 2] = a2;
            } else {                             // window (c1, c2, c3): the first output may fold (fl)
                float b0 = c1 - c2, b1 = c2, b2 = c3 - c2;
                if (colfold) { b0 = fmaf(fl, 2.f * c2 - c1, b0); b1 = fmaf(fl, c1, b1); b2 = fmaf(fl, c2, b2); }
                V[3 * xi] = b0; V[3 * xi + 1] = b1; V[3 * xi + 2] = b2;
            }
        }
    };
    f32x4 acc[9][2][2];
    auto mma = [&](const float (&a)[12], const float (&V)[9], int ex, int mt, bool first) {
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            if (first) acc[q][ex][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], V[q], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            else acc[q][ex][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], V[q], acc[q][ex][mt], 0, 0, 0);
        }
    };

    float a0[12], a1[12], V[9];
    f32x2 dl[3], dh[3];
    const int cof = cblk * 64 + 32 * ch + 4 * kq;      // this lane's input channels: cof + 16 mt + r (D rows 4 kq + r)
    __syncthreads();                                  // (drains the first requests: vmcnt(0))
    load_a(lds + aoff, 0, 0, a0);
    load_d(lds, 0, dl, dh);
    while (true) {
        int n, m0, n0;
        walk.origin<8, 32>(tile, n, m0, n0);
        {
            const int gbr = (m0 >> 1) + brow, gbc = (n0 >> 1) + t;          // global block row / column
            const int lastr = (p.Ho >> 1) - 1, lastc = (p.Wo >> 1) - 1;
            rt = !p.fold ? 0 : (ey == 1 && gbr == 0 ? 1 : (ey == 0 && gbr == lastr ? 2 : 0));
            fl = (p.fold && gbc == 0) ? 1.f : 0.f;
            fr = (p.fold && gbc == lastc) ? 1.f : 0.f;
            colfold = p.fold && (n0 == 0 || (n0 >> 1) + 16 > lastc);
        }
        // one chunk = two k-steps (4 gy channels each) x (ex, mt) in {0,1}^2: eight half-steps of 9 MFMAs; the A operand of a
        // half-step is read one half-step ahead; the patch of the next k-step is read once the column stage of ex = 1 has
        // consumed the current one (same registers)
        auto kstep = [&](const float* A, const float* Anext, const float* Xnext, int snext, bool first) {
            load_a(A, 0, 1, a1);
            __builtin_amdgcn_sched_barrier(0);
            transform_rows(dl, dh);
            transform_cols(dl, dh, 0, V);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, V, 0, 0, first);
            __builtin_amdgcn_sched_barrier(0);
            load_a(A, 1, 0, a0);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, V, 0, 1, first);
            __builtin_amdgcn_sched_barrier(0);
            load_a(A, 1, 1, a1);
            __builtin_amdgcn_sched_barrier(0);
            transform_cols(dl, dh, 1, V);
            __builtin_amdgcn_sched_barrier(0);
            load_d(Xnext, snext, dl, dh);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, V, 1, 0, first);
            __builtin_amdgcn_sched_barrier(0);
            load_a(Anext, 0, 0, a0);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, V, 1, 1, first);
            __builtin_amdgcn_sched_barrier(0);
        };
        auto chunk = [&](bool first) {
            const int u1 = u0 == 4 ? 0 : u0 + 1, u2 = u1 == 4 ? 0 : u1 + 1;
            const int rn = rc == 2 ? 0 : rc + 1;
            // the first k-step's tail reads this chunk's second half slab and raw slot: landed a chunk ago
            kstep(lds + u0 * D2G::UHALF + aoff, lds + u1 * D2G::UHALF + aoff, lds + rc * D2G::XS, 1, first);
            // everyone's requests for the NEXT chunk (issued one chunk ago) have landed; everyone has left the previous chunk's
            // raw slot and this chunk's first half slab
            ring_wait_landed<D2G>(cur.young_raw);                   // (never young: vmcnt(0))
            __builtin_amdgcn_sched_barrier(0);
            request(u0 == 0 ? 4 : u0 - 1, rc == 0 ? 2 : rc - 1);         // chunk after next: half slabs u0 + 4, u0 (mod 5); raw slot rc + 2 (mod 3)
            // (after the last chunk of the last tile the tail reads are stale and unused)
            kstep(lds + u1 * D2G::UHALF + aoff, lds + u2 * D2G::UHALF + aoff, lds + rn * D2G::XS, 0, false);
            u0 = u2;
            rc = rn;
        };
        chunk(true);
        for (int k = 1; k < K; ++k) chunk(false);
        // ---- epilogue: per column parity the output transform on channel pairs (columns with the lane's fold masks, rows with
        // the wave's variant), then one 16-byte store per (channel, output row): (n, ex) = (2C,0) (2C,1) (2C+1,0) (2C+1,1)
        const int mrow = m0 + 2 * brow;                      // parity-plane row of this lane's first output
        const int ncol = n0 + 2 * t;
        const __amdgpu_buffer_rsrc_t ro =
            __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + (size_t)n * p.Cs * HWin), 0, p.Cs * HWin * 4, 0x00020000);
        const bool in0 = ncol < p.Wo && mrow < p.Ho, in1 = in0 && mrow + 1 < p.Ho;
        const int vo0 = in0 ? (cof * HWin + (2 * mrow + ey) * Win + 2 * ncol) * 4 : RING_OOB;
        const int vo1 = in1 ? vo0 + 2 * Win * 4 : RING_OOB;
        // SKIP: frame b = n / T of gskip has the layout of frame n of gx (same offsets); plane (head, n) of a_up
        __amdgpu_buffer_rsrc_t rg = ro, ra = ro;
        int cpg_log2 = 0;
        if constexpr (SKIP) {
            const S2dParams C2S_AS4* kp = (const S2dParams C2S_AS4*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(kp));
            cpg_log2 = kp->cpg_log2;
            rg = __builtin_amdgcn_make_buffer_rsrc((void*)(kp->gskip + (size_t)(n / kp->T) * p.Cs * HWin), 0, p.Cs * HWin * 4, 0x00020000);
            ra = __builtin_amdgcn_make_buffer_rsrc((void*)(kp->a_up + (size_t)n * HWin), 0, kp->a_bytes, 0x00020000);
        }
        const f32x2 fl2 = {fl, fl}, fr2 = {fr, fr};
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 Y[2][2][2];                                         // [ex][output row i][output col j] on the channel pair
#pragma unroll
                for (int ex = 0; ex < 2; ++ex) {
                    f32x2 P0[3], P1[3];
#pragma unroll
                    for (int xi = 0; xi < 3; ++xi) {
                        f32x2 m[3];
#pragma unroll
                        for (int j = 0; j < 3; ++j) m[j] = (f32x2){acc[3 * xi + j][ex][mt][2 * h], acc[3 * xi + j][ex][mt][2 * h + 1]};
                        if (ex == 0) {                                    // the last output of the last block column may fold
                            P0[xi] = m[0] + m[1] + fr2 * (m[2] - m[1]);
                            P1[xi] = m[1] + m[2] - 2.f * fr2 * m[2];
                        } else {                                          // the first output of block column 0 may fold
                            P0[xi] = m[0] + m[1] - 2.f * fl2 * m[0];
                            P1[xi] = m[1] + m[2] + fl2 * (m[0] - m[1]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const f32x2* P = j == 0 ? P0 : P1;
                        if (rt == 0) { Y[ex][0][j] = P[0] + P[1]; Y[ex][1][j] = P[1] + P[2]; }
                        else if (rt == 1) { Y[ex][0][j] = P[1] - P[0]; Y[ex][1][j] = P[0] + P[2]; }
                        else { Y[ex][0][j] = P[0] + P[2]; Y[ex][1][j] = P[1] - P[2]; }
                    }
                }
                const int so = (16 * mt + 2 * h) * HWin * 4;
                f32x4 v[2][2];                                              // [channel of the pair][output row]
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 2; ++i) v[j][i] = (f32x4){Y[0][i][0][j], Y[1][i][0][j], Y[0][i][1][j], Y[1][i][1][j]};
                if constexpr (SKIP) {                                       // the six reads in flight before the first product
                    const int ho = (((cof + 16 * mt) >> cpg_log2) * p.N - cof) * HWin * 4;   // to the head plane of this lane's channel quad
#pragma unroll
                    for (int i = 0; i < 2; ++i) {                           // per output row: three reads in flight
                        const int vo = i == 0 ? vo0 : vo1;
                        const u32x4 au = __builtin_amdgcn_raw_buffer_load_b128(ra, vo == RING_OOB ? vo : vo + ho, 0, 0);
                        u32x4 o[2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) o[j] = __builtin_amdgcn_raw_buffer_load_b128(rg, i == 0 ? vo0 : vo1, so + j * HWin * 4, 0);
#pragma unroll
                        for (int j = 0; j < 2; ++j) v[j][i] += rounded_product(__builtin_bit_cast(f32x4, au), __builtin_bit_cast(f32x4, o[j]));
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                ring_store_rows(ro, vo0, vo1, so, HWin * 4, SKIP ? 0 : p.accumulate, v);
            }
        }
        if (cur.stile >= walk.ntotal) break;
        tile = cur.stile;
    }
}

void init_hook() {
    C2S_RAISE_LDS(conv_s2dgrad_kernel<false>);
    C2S_RAISE_LDS(conv_s2dgrad_kernel<true>);
}
C2sInitRegistrar registrar(init_hook);

}  // namespace

// d: the FORWARD convolution's geometry seen from the gradient: C0 = gy channels (the forward Cout), Hin x Win = the gy plane
// (forward output), Cout / CoutP = the forward input channels of this source, Hout x Wout = 2 Hin x 2 Win = the gx plane
extern "C" int c2s_conv4x4s2_dgrad_winograd_supported(const c2s_conv_desc* d) {
    return d && d->KH == 4 && d->KW == 4 && d->S == 2 && d->pad_y == 1 && d->pad_x == 1 && d->C1 == 0 && d->C0 % 8 == 0 &&
           d->C0 >= 24 && d->Hout == 2 * d->Hin && d->Wout == 2 * d->Win && d->Hin % 2 == 0 && d->Win % 2 == 0 &&
           d->Win >= 32 && d->Hin >= 8 && d->CoutP % 64 == 0 && d->N <= ring_max_frames<D2G>();
}

namespace {

// a_up == NULL: gx (+)= the gradient; else gx = the gradient + round(a_up * gskip) (the descriptor's accumulate must be 0)
int s2dgrad(const c2s_conv_desc* d, const float* gy, const float* upk, float* gx, const int* valid, const float* a_up,
            const float* gskip, int T, int n_head, void* stream) {
    if (int rc = ring_check("conv4x4s2_dgrad_winograd", d, gy && upk && gx, ring_max_frames<D2G>(), RING_OOB, true)) return rc;
    C2S_REQUIRE(c2s_conv4x4s2_dgrad_winograd_supported(d), "conv4x4s2_dgrad_winograd: data gradient of a 4x4 stride 2 pad 1 convolution, gy channels a multiple of 8 (>= 24), even gy planes at least 32 wide and 8 high, CoutP %% 64");
    C2S_REQUIRE(d->Cout > 0 && d->CoutP >= d->Cout, "conv4x4s2_dgrad_winograd: bad channels");
    S2dParams p;
    p.src = gy; p.upk = upk; p.out = gx; p.valid = valid;
    p.Kc = d->C0; p.Ho = d->Hin; p.Wo = d->Win; p.Cs = d->Cout; p.CsP = d->CoutP;
    p.fold = d->reflect_adjoint; p.accumulate = d->accumulate;
    p.tiles_x = cdiv(d->Win, 32);
    p.tiles = p.tiles_x * cdiv(d->Hin, 8);
    p.N = d->N;
    p.nchunks = d->C0 / 8;
    p.a_up = a_up; p.gskip = gskip; p.T = T; p.cpg_log2 = 0;
    p.a_bytes = (int)((((long)n_head - 1) * d->N + 1) * d->Hout * d->Wout * 4);
    if (a_up != nullptr) {
        C2S_REQUIRE(gskip && c2s_conv4x4s2_dgrad_winograd_skip_supported(d, n_head, T) && d->accumulate == 0,
                    "conv4x4s2_dgrad_winograd_skip: needs Cout / n_head in {4, 8, 16}, N a multiple of T, accumulate 0 and "
                    "(CoutP / (Cout / n_head) + 1) N Hout Wout floats below 2 GB");
        while ((d->Cout / n_head) >> (p.cpg_log2 + 1)) ++p.cpg_log2;
    }
    const dim3 grid = ring_grid(2 * (d->CoutP / 64), (long)d->N * p.tiles, 1);
    const size_t ldsb = ring_lds_bytes<D2G>(d->N);
    if (a_up != nullptr) hipLaunchKernelGGL(conv_s2dgrad_kernel<true>, grid, dim3(512), ldsb, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(conv_s2dgrad_kernel<false>, grid, dim3(512), ldsb, (hipStream_t)stream, p);
    C2S_CHECK_LAUNCH("conv4x4s2_dgrad_winograd");
    return C2S_OK;
}

}  // namespace

extern "C" int c2s_conv4x4s2_dgrad_winograd(const c2s_conv_desc* d, const float* gy, const float* upk, float* gx,
                                            const int* valid, void* stream) {
    return s2dgrad(d, gy, upk, gx, valid, nullptr, nullptr, 1, 1, stream);
}

// the same gradient with the skip term of the temporal aggregation added in the epilogue: gx[n] = gradient + round(a_up[g, n] *
// gskip[n / T]) with g the head of the channel, a_up [n_head][N][Hout][Wout] as c2s_temporal_aggregate_bwd_skip stores it and
// gskip [N / T][Cout][Hout][Wout]; gx is not read.  A lane's four channels must share a head: Cout / n_head in {4, 8, 16}
extern "C" int c2s_conv4x4s2_dgrad_winograd_skip_supported(const c2s_conv_desc* d, int n_head, int T) {
    if (!c2s_conv4x4s2_dgrad_winograd_supported(d) || n_head <= 0 || T <= 0 || d->N % T != 0 || d->Cout % n_head != 0) return 0;
    const int cpg = d->Cout / n_head;
    return (cpg == 4 || cpg == 8 || cpg == 16) &&
           (long)(d->CoutP / cpg + 1) * d->N * d->Hout * d->Wout * 4 < 0x7FFF0000L;
}

extern "C" int c2s_conv4x4s2_dgrad_winograd_skip(const c2s_conv_desc* d, const float* gy, const float* upk, float* gx,
                                                 const int* valid, const float* a_up, const float* gskip, int n_head, int T,
                                                 void* stream) {
    C2S_REQUIRE(a_up && gskip, "conv4x4s2_dgrad_winograd_skip: null pointer");
    return s2dgrad(d, gy, upk, gx, valid, a_up, gskip, T, n_head, stream);
}
