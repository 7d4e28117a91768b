// Implicit-GEMM convolution for gfx950 on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32).
//
// GEMM view (per frame n):   D[cout][pos] = sum_{tap, cin} Wpk[tap][cin][cout] * In[cin][gather(pos, tap)]
//   A operand (MFMA rows i) = output channel  -> accumulator rows are channels,
//   B operand (MFMA cols j) = output position -> lanes 0..31 of a store hit 32 consecutive x of one
//                                               NCHW row: 128-byte coalesced stores.
// Workgroup = 256 threads = 4 waves.  Tile = 8 position fragments of 32 positions (FR rows x FC cols,
// FC = 2^log2fc adapts to narrow planes: 128 -> 1x32, 16 -> 2x16) x COT = 32*MF output channels.
// Wave w owns position fragments 2w, 2w+1 and all MF channel fragments: MF*2 accumulators of 16 VGPRs.
// K loop: input channels in chunks of CK staged in LDS together with the [tap][CK][COT] weight slab;
// the gather offsets of a thread's staging elements are computed once per tile (reflection included)
// and kept in registers, so the per-chunk staging is load + ds_write only.
//
//
// Split tiles (SP = 2, 4; MF = 1) for launches too small to fill the GPU (the decoder and head run on N = batch frames:
// a 32-channel 3x3 layer at 64x64, N = 4 is 64 workgroups on 256 CUs, each wave walking the whole K loop with two MFMAs
// per k-step).  SP = 2: the tile is 4 position fragments, a wave owns ONE; SP = 4: 2 fragments, a workgroup of 2 waves.
// The grid grows SP-fold and a wave issues half the MFMAs; its operand reads run two k-steps ahead, since one MFMA no
// longer covers an LDS round trip.  Every output element is still the same chain of MFMAs over the same k-steps in the
// same order, so the result is BIT-IDENTICAL to the unsplit tile's: the choice may depend on the frame count without
// making a sample's result depend on its batch (tests pin that bit for bit).  (Splitting the K loop over the waves of a
// tile, the first form of this, was faster again on the smallest launches but rounds differently at every split, which
// breaks exactly that: DESIGN 8.)  c2s_conv_igemm_split is the rule that picks SP.
//
// Reference call sites replaced: nn.Conv2d / nn.ConvTranspose2d in src/backbones/conv.py:70-80,
// 263-271,378-390 and their convolution_backward-input.
#include "conv_tile.h"

namespace {

constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int plane_for(int K, int S, int log2fc, int NF) {      // NF = position fragments of the tile (8 / SP)
    return ((NF * (32 >> log2fc) - 1) * S + K) * (((1 << log2fc) - 1) * S + K);
}
constexpr int max_plane(int K, int S, int NF) {
    return cmax(cmax(plane_for(K, S, 2, NF), plane_for(K, S, 3, NF)), cmax(plane_for(K, S, 4, NF), plane_for(K, S, 5, NF)));
}

// channels per LDS chunk: enough MFMA k-steps per barrier pair (>= 16) without growing the prefetch registers
constexpr int chunk_channels(int K) { return K == 1 ? 16 : (K == 2 ? 8 : (K >= 4 ? 2 : 4)); }

template <int K, int S, int SP = 1>
struct Cfg {
    static constexpr int CK = chunk_channels(K);
    static constexpr int NT = K * K;
    static constexpr int NTHR = SP == 4 ? 128 : 256;             // threads of a workgroup
    static constexpr int MAXE = (CK * max_plane(K, S, 8 / SP) + NTHR - 1) / NTHR;
};

template <int K, int S, int MF, bool ADJ, int SP = 1>
__global__ __launch_bounds__((Cfg<K, S, SP>::NTHR)) void conv_igemm_kernel(TileParams p) {
    static_assert(SP == 1 || ((SP == 2 || SP == 4) && MF == 1), "the split tiles exist for 32-channel tiles");
    constexpr int CK = Cfg<K, S, SP>::CK;
    constexpr int NT = Cfg<K, S, SP>::NT;
    constexpr int NF = 8 / SP;                   // position fragments of the tile
    constexpr int NQ = SP == 1 ? 2 : 1;          // fragments (accumulators per channel fragment) of a wave
    constexpr int LA = SP == 1 ? 1 : 2;          // k-steps the operand reads run ahead of the MFMAs
    constexpr int COT = 32 * MF;
    constexpr int NS = NT * (CK / 2);            // MFMA k-steps per chunk
    typedef TileStage<CK, Cfg<K, S, SP>::MAXE, Cfg<K, S, SP>::NTHR, NT, COT> Stage;
    extern __shared__ float lds[];

    int bxi, n;
    tile_frame_order(bxi, n);
    if (p.valid != nullptr && p.valid[n] == 0) return;

    const int FC = 1 << p.log2fc, FR = 32 >> p.log2fc;
    const int tile_h = NF * FR, tile_w = FC;
    const int rows = (tile_h - 1) * S + K, cols = (tile_w - 1) * S + K;
    const int plane = rows * cols;
    float* Xl = lds;                 // [2][ [CK][plane] | [NT][CK][COT] ]
    float* Wl = lds + tile_x_floats(CK, plane);
    const int BUF = tile_buf_floats(CK, plane, Stage::WFLOATS);

    const int tyi = bxi / p.tiles_x, txi = bxi % p.tiles_x;
    const int oy0 = tyi * tile_h, ox0 = txi * tile_w;
    const int co0 = blockIdx.y * COT;
    const int tid = threadIdx.x;

    Stage st;
    st.init(tid, n, p.src0, p.src1, p.wpk, p.C0, p.C1, p.Hin, p.Win, p.CoutP, co0, plane, cols, oy0 * S - p.pad_y,
            ox0 * S - p.pad_x, p.pad_y, p.pad_x, p.pad_mode);

    const int wave = tid >> 6;
    const TileLane ln = tile_lane(tid, p.log2fc);
    const int li = ln.li, lk = ln.lk, fy = ln.fy, fx = ln.fx;
    int boff[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int f = NQ * wave + q;
        boff[q] = lk * plane + ((f * FR + fy) * S) * cols + fx * S;
    }
    const int aoff = lk * COT + li;

    // reflect adjoint: per-lane masks of the border positions this lane owns
    float mxlo[NQ] = {}, mxhi[NQ] = {}, mylo[NQ] = {}, myhi[NQ] = {};
    if constexpr (ADJ) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int f = NQ * wave + q;
            const int oy = oy0 + f * FR + fy, ox = ox0 + fx;
            mxlo[q] = ox == p.ax_lo ? 1.f : 0.f;
            mxhi[q] = ox == p.ax_hi ? 1.f : 0.f;
            mylo[q] = oy == p.ay_lo ? 1.f : 0.f;
            myhi[q] = oy == p.ay_hi ? 1.f : 0.f;
        }
    }

    f32x16 acc[MF][NQ];
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;

    // operands of k-step s = (tap t, channel pair cp)
    struct Ops {
        float a[MF], b[NQ];
    };
    auto load_ops = [&](const float* Xl, const float* Wl, int s_, Ops& o) {
        const int t = s_ / (CK / 2), cp = s_ % (CK / 2);
        const int ky = t / K, kx = t % K;
#pragma unroll
        for (int m = 0; m < MF; ++m) o.a[m] = Wl[(t * CK + 2 * cp) * COT + aoff + m * 32];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int ad = boff[q] + 2 * cp * plane + ky * cols + kx;
            float v = Xl[ad];
            if constexpr (ADJ) {
                // fold of the reflected halo: offsets of at most K-1, always inside the staged tile
                const bool xl = kx == K - 1, xh = kx == 0, yl = ky == K - 1, yh = ky == 0;
                const int dx = xl ? -p.dx_lo : p.dx_hi;
                if (xl || xh) {                      // branch-free (0 / 1 lane masks): see conv_xpair.hip
                    const float mx = xl ? mxlo[q] : mxhi[q];
                    v = fmaf(mx, Xl[ad + dx], v);
                }
                if (yl || yh) {
                    const float my = yl ? mylo[q] : myhi[q];
                    const int dy = (yl ? -p.dy_lo : p.dy_hi) * cols;
                    v = fmaf(my, Xl[ad + dy], v);
                    if (xl || xh) {
                        const float mx = xl ? mxlo[q] : mxhi[q];
                        v = fmaf(my * mx, Xl[ad + dy + dx], v);
                    }
                }
            }
            o.b[q] = v;
        }
    };
    tile_chunk_loop<NS, LA, NS / 2, Ops>(st, Xl, Wl, BUF, load_ops, [&](const Ops& o) {
#pragma unroll
        for (int m = 0; m < MF; ++m)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.a[m], o.b[q], acc[m][q], 0, 0, 0);
    });

    // ---- epilogue: one float per channel at (oy*osy+ooy, ox*osx+oox)
    const size_t outHW = (size_t)p.OutH * p.OutW;
    float* on = p.out + (size_t)n * p.Cout * outHW;
    // (one call per fragment, not a loop over q: out of a loop hipcc hoists the sixteen 64-bit channel offsets, 32 VGPRs)
    auto store = [&](int q) __attribute__((always_inline)) {
        const int f = NQ * wave + q;
        const int oy = oy0 + f * FR + fy, ox = ox0 + fx;
        if (oy >= p.Hout || ox >= p.Wout) return;
        const size_t sp = (size_t)(oy * p.osy + p.ooy) * p.OutW + (ox * p.osx + p.oox);
        tile_store<MF>(on, sp, outHW, co0, lk, p.Cout, p.bias, p.accumulate,
                              [&](int m, int r) __attribute__((always_inline)) { return acc[m][q][r]; });
    };
    store(0);
    if constexpr (NQ == 2) store(1);
}

template <int K, int S, int MF, bool ADJ, int SP = 1>
int launch_conv(const TileParams& p, int N, int tiles, hipStream_t st) {
    constexpr int CK = Cfg<K, S, SP>::CK;
    constexpr int NT = Cfg<K, S, SP>::NT;
    const size_t lds = tile_lds_bytes(CK, plane_for(K, S, p.log2fc, 8 / SP), NT * CK * 32 * MF);
    dim3 grid(tiles, p.CoutP / (32 * MF), N);
    hipLaunchKernelGGL((conv_igemm_kernel<K, S, MF, ADJ, SP>), grid, dim3(Cfg<K, S, SP>::NTHR), lds, st, p);
    C2S_CHECK_LAUNCH("conv_igemm");
    return C2S_OK;
}

// the (K, S, reflect adjoint) the kernel is built for: the dispatch and the LDS limits below
#define C2S_IGEMM_KINDS(X) \
    X(3, 1, false) X(3, 1, true) X(1, 1, false) X(2, 1, false) X(2, 1, true) X(4, 2, false) X(2, 2, false) X(6, 2, false)

void init_hook() {
#define C2S_RAISE(K_, S_, A_)                              \
    C2S_RAISE_LDS((conv_igemm_kernel<K_, S_, 1, A_>));     \
    C2S_RAISE_LDS((conv_igemm_kernel<K_, S_, 2, A_>));     \
    C2S_RAISE_LDS((conv_igemm_kernel<K_, S_, 1, A_, 2>));  \
    C2S_RAISE_LDS((conv_igemm_kernel<K_, S_, 1, A_, 4>));
    C2S_IGEMM_KINDS(C2S_RAISE)
#undef C2S_RAISE
}
C2sInitRegistrar registrar(init_hook);

// the workgroups of a launch at split sp (32-channel tiles)
long split_wgs(const c2s_conv_desc* d, int sp) {
    return (long)tile_count(d->Hout, d->Wout, tile_log2fc(d->Wout), 8 / sp) * d->N * (d->CoutP / 32);
}
// C2S_IGEMM_SPLIT=1|2|4 forces the split (A/B runs, tests); anything else: the rule
int forced_split() {
    const char* e = getenv("C2S_IGEMM_SPLIT");
    if (e == nullptr || e[0] == 0 || e[1] != 0) return 0;
    return e[0] == '1' ? 1 : (e[0] == '2' ? 2 : (e[0] == '4' ? 4 : 0));
}

}  // namespace

// The split of a launch (1, 2 or 4), host arithmetic only.  1 where the 256-position tiles already put two workgroups
// on every CU (every large launch); otherwise the smallest split that does, else 4.  Never decreases as N shrinks; the
// result of a launch does not depend on it (bit-identical tiles), only its duration does.
extern "C" int c2s_conv_igemm_split(const c2s_conv_desc* d, int cus) {
    if (d == nullptr || d->N <= 0 || d->C0 <= 0 || d->C1 < 0 || d->CoutP < 32 || d->Hout <= 0 || d->Wout <= 0 || d->KH <= 0) return 1;
    if (cus <= 0) cus = c2s_cus();
    if (split_wgs(d, 1) >= 2L * cus) return 1;
    return split_wgs(d, 2) >= 2L * cus ? 2 : 4;
}

extern "C" int c2s_conv_igemm(const c2s_conv_desc* d, const float* src0, const float* src1, const float* wpk,
                              const float* bias, float* out, const int* valid, void* stream) {
    if (const int rc = tile_check("conv_igemm", d, src0 && wpk && out)) return rc;
    C2S_REQUIRE(d->Cout > 0, "conv_igemm: CoutP must be a multiple of 32");      // (the message this case has always had)
    C2S_REQUIRE(d->N > 0 && d->C0 > 0 && d->C1 >= 0 && (d->C1 == 0 || src1), "conv_igemm: bad channels");
    C2S_REQUIRE(d->KH == d->KW, "conv_igemm: square kernels only");
    // (a chunk of the K loop never straddles the two sources: decoder widths such as 24 and 40 reach the 3x3 layers)
    C2S_REQUIRE(d->C1 == 0 || d->C0 % chunk_channels(d->KH) == 0,
                "conv_igemm: with two sources C0 must be a multiple of the channel chunk (16 for 1x1, 8 for 2x2, 4 for 3x3, 2 above)");
    C2S_REQUIRE((long)d->Hin * d->Win < (1 << 20), "conv_igemm: input plane too large");
    C2S_REQUIRE(d->Hout > 0 && d->Wout > 0, "conv_igemm: empty output");
    C2S_REQUIRE((d->Hout - 1) * d->osy + d->ooy < d->OutH && (d->Wout - 1) * d->osx + d->oox < d->OutW,
                "conv_igemm: output placement exceeds the output plane");
    if (d->pad_mode == C2S_PAD_REFLECT)
        C2S_REQUIRE(d->pad_y < d->Hin && d->pad_x < d->Win, "conv_igemm: reflect padding needs pad < size");
    TileParams p;
    tile_fill(p, d, src0, src1, wpk, bias, out, valid);
    if (d->reflect_adjoint == 2) {
        // parity sub-kernel (3x3, pad 1, output rows 2*a + parity) of the dgrad of conv6x6s2(reflect pad 2); per dimension
        // the input gradient of padded rows -1 / -2 / H / H+1 is the sub-kernel evaluated one row beyond either end:
        //   parity 0: position 1 / tap 2 additionally reads input tap position - 2, position Ho-1 / tap 0 reads + 1
        //   parity 1: position 0 / tap 2 reads tap position - 1,                  position Ho-2 / tap 0 reads + 2
        C2S_REQUIRE(d->pad_mode == C2S_PAD_ZEROS && d->S == 1 && d->KH == 3 && d->pad_y == 1 && d->pad_x == 1 &&
                    d->osy == 2 && d->osx == 2 && d->ooy >= 0 && d->ooy <= 1 && d->oox >= 0 && d->oox <= 1 &&
                    d->Hin == d->Hout && d->Win == d->Wout && d->Hin >= 2 && d->Win >= 2,
                    "conv_igemm: reflect_adjoint 2 applies to the parity launches of the 6x6 stride-2 data gradient");
        p.ay_lo = d->ooy == 0 ? 1 : 0;   p.dy_lo = d->ooy == 0 ? 2 : 1;
        p.ay_hi = d->Hout - 1 - d->ooy;  p.dy_hi = d->ooy == 0 ? 1 : 2;
        p.ax_lo = d->oox == 0 ? 1 : 0;   p.dx_lo = d->oox == 0 ? 2 : 1;
        p.ax_hi = d->Wout - 1 - d->oox;  p.dx_hi = d->oox == 0 ? 1 : 2;
    } else if (d->reflect_adjoint) {
        C2S_REQUIRE(d->pad_mode == C2S_PAD_ZEROS && d->S == 1 && (d->KH == 3 || d->KH == 2),
                    "conv_igemm: reflect_adjoint applies to the zero-padded 3x3 / 2x2-parity data-gradient launches");
        C2S_REQUIRE(d->Hin >= 2 && d->Win >= 2, "conv_igemm: reflect_adjoint needs planes of at least 2");
        if (d->KH == 3) {
            // dgrad of conv3x3(reflect pad 1): g_x[1] += w[0] g_y[0] ; g_x[H-2] += w[2] g_y[H-1]
            // (flipped taps: position 1 / tap 2 reads input 0 = tap position - 2; position H-2 / tap 0 reads H-1 = +2)
            // On a 3-pixel axis lo == hi == 1: the two rules sit on different taps of that position (tap 2 reads row 2 and
            // adds row 0, tap 0 reads row 0 and adds row 2), and the kernel keeps one mask per rule, so both apply.
            C2S_REQUIRE(d->pad_y == 1 && d->pad_x == 1 && d->Hin == d->Hout && d->Win == d->Wout, "conv_igemm: bad 3x3 adjoint geometry");
            p.ay_lo = 1; p.ay_hi = d->Hout - 2;
            p.ax_lo = 1; p.ax_hi = d->Wout - 2;
        } else {
            // parity sub-kernel of the dgrad of conv4x4s2(reflect pad 1); parity = 1 - pad:
            // parity 1 (pad 0): position 0 / tap 1 additionally reads input 0; parity 0 (pad 1): position Ho-1 / tap 0 reads Ho-1
            if (d->pad_y == 0) p.ay_lo = 0; else p.ay_hi = d->Hout - 1;
            if (d->pad_x == 0) p.ax_lo = 0; else p.ax_hi = d->Wout - 1;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int cus = c2s_cus();
    // launches that leave CUs empty run on smaller tiles with one fragment per wave (c2s_conv_igemm_split)
    const int forced = forced_split();
    const int sp = forced ? forced : c2s_conv_igemm_split(d, cus);
    const int tiles = tile_count(d->Hout, d->Wout, p.log2fc, 8 / sp);
    const bool wide = sp == 1 && tile_wide(d->CoutP, tiles, d->N, cus);
#define C2S_DISPATCH(K_, S_, A_)                                                   \
    if (d->KH == K_ && d->S == S_ && (p.adj != 0) == A_) {                         \
        if (sp == 2) return launch_conv<K_, S_, 1, A_, 2>(p, d->N, tiles, st);     \
        if (sp == 4) return launch_conv<K_, S_, 1, A_, 4>(p, d->N, tiles, st);     \
        return wide ? launch_conv<K_, S_, 2, A_>(p, d->N, tiles, st) : launch_conv<K_, S_, 1, A_>(p, d->N, tiles, st); \
    }
    C2S_IGEMM_KINDS(C2S_DISPATCH)
#undef C2S_DISPATCH
    c2s_set_error("conv_igemm: unsupported (K=%d,S=%d)", d->KH, d->S);
    return C2S_EINVAL;
}
