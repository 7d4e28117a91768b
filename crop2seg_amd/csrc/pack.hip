// Weight packing: every packed layout the convolution kernels read, written by one device routine per layout.
//
// A PackJob describes one pack: the filter element (o, c, tap t) is src[o * so + c * sc + taps[t]], o < cout output channels
// padded to coutP, c < cin input channels.  Thread e of a job computes item e of its layout (pack_items) and writes every
// float that item owns, padding included, so a buffer holds the same bits whichever launcher filled it:
//   pack_one_kernel    one job passed by value: the c2s_pack_weights* exports (every forward outside a recorded plan)
//   pack_batch_kernel  a device table of jobs in one launch: the per-step pack plan (c2s_pack_job_fill, c2s_pack_batch)
#include "common.h"

namespace {

enum PackKind {
    PACK_TAPS = 0,      // wpk[tap][cin][coutP]: implicit GEMM, x-pair, parity sub-convolutions, first layer
    PACK_WINO = 1,      // Winograd U of conv_winograd.hip
    PACK_WINO16 = 2,    // Winograd U of conv_winograd16.hip
    PACK_S2WINO = 3,    // F(2x2,2x2) parity U of conv_s2wino.hip
    PACK_S2DGRAD = 4,   // F(2x2,2x2) data-gradient U of conv_s2dgrad.hip
    PACK_KINDS = 5
};

struct PackJob {
    const float* src;
    float* dst;
    long so, sc;
    int cin, cout, coutP, ntaps;
    int kind;            // PackKind
    int block_start;     // first block of this job in a batch table
    int taps[C2S_MAX_TAPS];
};

constexpr int PACK_THREADS = 256;
constexpr int PACK_MAX_BLOCKS = 2048;   // single packs: grid-stride beyond this

// threads (items) of a job: one output element (kind 0), one (c, o) pair (1, 2), one (c, parity, o) triple (3, 4)
__host__ __device__ inline long pack_items(int kind, int cin, int coutP, int ntaps) {
    switch (kind) {
    case PACK_TAPS: return (long)ntaps * cin * coutP;
    case PACK_WINO: return (long)((cin + WN_CK - 1) / WN_CK) * WN_CK * coutP;
    case PACK_WINO16: return (long)((cin + W16_CK - 1) / W16_CK) * W16_CK * coutP;
    case PACK_S2WINO: return (long)((cin + 1) / 2) * 2 * 4 * coutP;
    case PACK_S2DGRAD: return 4L * cin * coutP;
    default: return 0;
    }
}

size_t pack_floats(int kind, int cin, int coutP, int ntaps) {
    static const int per_item[PACK_KINDS] = {1, WN_USLAB / (WN_CK * 64), W16_UP, S2_UP, D2_UP};
    return (size_t)pack_items(kind, cin, coutP, ntaps) * per_item[kind];
}

// G g Gt of the 3x3 filter of (c, o), zero past the real counts.
//   kind 1: [cout block][chunk][xn 16][c WN_CK][o 64]
//   kind 2: [cout block][chunk][c W16_CK][xi 4][o 64][nu 4]: the 16 lanes of an MFMA operand read (16 consecutive output
//           channels, one xi) touch 256 contiguous bytes -- conflict-free without padding per (c, o)
__device__ __forceinline__ void pack_winograd(const PackJob& j, long e, bool wide) {
    const int o = (int)(e % j.coutP), c = (int)(e / j.coutP);
    const bool real = o < j.cout && c < j.cin;
    float g[3][3];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = real ? j.src[o * j.so + c * j.sc + j.taps[k]] : 0.f;
    float t[4][3];                                  // G g
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        t[0][q] = g[0][q];
        t[1][q] = 0.5f * (g[0][q] + g[1][q] + g[2][q]);
        t[2][q] = 0.5f * (g[0][q] - g[1][q] + g[2][q]);
        t[3][q] = g[2][q];
    }
    float* base;
    int xi_stride, nu_stride;
    if (wide) {
        const int nchunks = (j.cin + W16_CK - 1) / W16_CK;
        base = j.dst + (((size_t)(o >> 6) * nchunks + c / W16_CK) * W16_CK + c % W16_CK) * 64 * W16_UP + (size_t)(o & 63) * 4;
        xi_stride = 64 * 4;
        nu_stride = 1;
    } else {
        const int nchunks = (j.cin + WN_CK - 1) / WN_CK;
        base = j.dst + ((size_t)(o >> 6) * nchunks + c / WN_CK) * WN_USLAB + (c % WN_CK) * 64 + (o & 63);
        xi_stride = 4 * WN_CK * 64;
        nu_stride = WN_CK * 64;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        base[i * xi_stride + 0 * nu_stride] = t[i][0];
        base[i * xi_stride + 1 * nu_stride] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
        base[i * xi_stride + 2 * nu_stride] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
        base[i * xi_stride + 3 * nu_stride] = t[i][2];
    }
}

// U = G g Gt of a 2x2 sub-filter g: the 9 points at base[0..8], zeros up to the entry's `up` floats
__device__ __forceinline__ void store_f22(float* base, const float (&g)[2][2], int up) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float u0 = i == 0 ? g[0][0] : (i == 1 ? g[0][0] + g[1][0] : g[1][0]);
        const float u1 = i == 0 ? g[0][1] : (i == 1 ? g[0][1] + g[1][1] : g[1][1]);
        base[i * 3 + 0] = u0;
        base[i * 3 + 1] = u0 + u1;
        base[i * 3 + 2] = u1;
    }
    for (int i = 9; i < up; ++i) base[i] = 0.f;
}

// the four 2x2 parity sub-filters of the 4x4 filter w[ky][kx] = taps[ky * 4 + kx]: parity 0 of a dimension uses taps (1, 3),
// parity 1 taps (0, 2); stored [cout block][chunk][2 c][4 parities][64 o][S2_UP]
__device__ __forceinline__ void pack_s2wino(const PackJob& j, long e) {
    const int nchunks = (j.cin + 1) / 2;
    const int o = (int)(e % j.coutP);
    const int par = (int)((e / j.coutP) & 3), c = (int)(e / j.coutP / 4);
    const int py = par >> 1, px = par & 1;
    const bool real = o < j.cout && c < j.cin;
    float g[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ky = (py == 0 ? 1 : 0) + 2 * a, kx = (px == 0 ? 1 : 0) + 2 * b;
            g[a][b] = real ? j.src[o * j.so + c * j.sc + j.taps[ky * 4 + kx]] : 0.f;
        }
    store_f22(j.dst + ((((size_t)(o >> 6) * nchunks + (c >> 1)) * 2 + (c & 1)) * 4 + par) * 64 * S2_UP + (size_t)(o & 63) * S2_UP,
              g, S2_UP);
}

// the 2x2 sub-filter of output parity (ey, ex) of the 4x4 stride-2 data gradient: rows ky = (3, 1) for ey = 0, (2, 0) for
// ey = 1 (columns likewise).  Here cin = gy channels k (a multiple of 8), cout / coutP = input channels c: the element
// w(k, c, ky, kx) = src[c * so + k * sc + taps[ky * 4 + kx]]; stored [ey][cin block][chunk][2 k-steps][4 k][128 = ex * 64 + c][D2_UP]
__device__ __forceinline__ void pack_s2dgrad(const PackJob& j, long e) {
    const int c = (int)(e % j.coutP);
    const int k = (int)((e / j.coutP) % j.cin);
    const int par = (int)(e / j.coutP / j.cin);
    const int ey = par >> 1, ex = par & 1;
    const bool real = c < j.cout;
    float g[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ky = (ey == 0 ? 3 : 2) - 2 * a, kx = (ex == 0 ? 3 : 2) - 2 * b;
            g[a][b] = real ? j.src[c * j.so + k * j.sc + j.taps[ky * 4 + kx]] : 0.f;
        }
    const int cblocks = j.coutP / 64, nchunks = j.cin / 8;
    store_f22(j.dst + ((((size_t)(ey * cblocks + (c >> 6)) * nchunks + (k >> 3)) * 2 + ((k >> 2) & 1)) * 4 + (k & 3)) * 128 * D2_UP +
                  (size_t)(ex * 64 + (c & 63)) * D2_UP,
              g, D2_UP);
}

// item e < pack_items(j) of job j (kind = j.kind)
__device__ __forceinline__ void pack_item(const PackJob& j, long e, int kind) {
    switch (kind) {
    case PACK_TAPS: {
        const int o = (int)(e % j.coutP);
        const long tc = e / j.coutP;
        const int c = (int)(tc % j.cin), t = (int)(tc / j.cin);
        j.dst[e] = o < j.cout ? j.src[o * j.so + c * j.sc + j.taps[t]] : 0.f;
        break;
    }
    case PACK_WINO:
    case PACK_WINO16: pack_winograd(j, e, kind == PACK_WINO16); break;
    case PACK_S2WINO: pack_s2wino(j, e); break;
    case PACK_S2DGRAD: pack_s2dgrad(j, e); break;
    }
}

// (one instance per kind: the code of a single layout, as fast as the per-layout kernels it replaced)
template <int KIND>
__global__ void pack_one_kernel(PackJob j) {
    const long total = pack_items(KIND, j.cin, j.coutP, j.ntaps);
    for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) pack_item(j, e, KIND);
}

__global__ void pack_batch_kernel(const PackJob* __restrict__ jobs, int njobs) {
    int i = 0;
    while (i + 1 < njobs && (int)blockIdx.x >= jobs[i + 1].block_start) ++i;      // <= ~64 jobs: linear scan
    const PackJob& j = jobs[i];
    const long e = (long)(blockIdx.x - j.block_start) * blockDim.x + threadIdx.x;
    if (e < pack_items(j.kind, j.cin, j.coutP, j.ntaps)) pack_item(j, e, j.kind);
}

// Checks a job against what its kind reads and writes, then fills it
int pack_job_init(PackJob* j, const char* who, int kind, const float* src, float* dst, int cin, int cout, int coutP, int ntaps,
                  long so, long sc, const int* taps, int block_start) {
    C2S_REQUIRE(src && dst && taps, "%s: null pointer", who);
    C2S_REQUIRE(kind >= 0 && kind < PACK_KINDS, "%s: unknown layout %d", who, kind);
    C2S_REQUIRE(cin > 0 && cout > 0 && coutP >= cout, "%s: bad channel counts", who);
    if (kind == PACK_TAPS) {
        C2S_REQUIRE(ntaps >= 1 && ntaps <= C2S_MAX_TAPS, "%s: bad tap count", who);
        C2S_REQUIRE(coutP % 32 == 0, "%s: CoutP must be a multiple of 32", who);
    } else {
        C2S_REQUIRE(ntaps == (kind <= PACK_WINO16 ? 9 : 16), "%s: a 3x3 (Winograd) or 4x4 (stride 2) filter", who);
        C2S_REQUIRE(coutP % 64 == 0, "%s: CoutP must be a multiple of 64", who);
        C2S_REQUIRE(kind != PACK_S2DGRAD || cin % 8 == 0, "%s: gy channels must be a multiple of 8", who);
    }
    j->src = src; j->dst = dst; j->so = so; j->sc = sc;
    j->cin = cin; j->cout = cout; j->coutP = coutP; j->ntaps = ntaps; j->kind = kind; j->block_start = block_start;
    for (int i = 0; i < C2S_MAX_TAPS; ++i) j->taps[i] = i < ntaps ? taps[i] : 0;
    return C2S_OK;
}

int pack_one(const char* who, int kind, const float* src, float* dst, int cin, int cout, int coutP, int ntaps, long so, long sc,
             const int* taps, void* stream) {
    PackJob j;
    const int rc = pack_job_init(&j, who, kind, src, dst, cin, cout, coutP, ntaps, so, sc, taps, 0);
    if (rc != C2S_OK) return rc;
    static void (*const kernels[PACK_KINDS])(PackJob) = {pack_one_kernel<PACK_TAPS>, pack_one_kernel<PACK_WINO>,
        pack_one_kernel<PACK_WINO16>, pack_one_kernel<PACK_S2WINO>, pack_one_kernel<PACK_S2DGRAD>};
    const int blocks = cdiv(pack_items(kind, cin, coutP, ntaps), PACK_THREADS);
    hipLaunchKernelGGL(kernels[kind], dim3(blocks < PACK_MAX_BLOCKS ? blocks : PACK_MAX_BLOCKS), dim3(PACK_THREADS), 0,
                       (hipStream_t)stream, j);
    C2S_CHECK_LAUNCH(who);
    return C2S_OK;
}

}  // namespace

extern "C" int c2s_pack_weights(const float* src, float* wpk, int cin, int cout, int coutP, int ntaps, long stride_o,
                                long stride_c, const int* host_tap_off, void* stream) {
    return pack_one("pack_weights", PACK_TAPS, src, wpk, cin, cout, coutP, ntaps, stride_o, stride_c, host_tap_off, stream);
}

extern "C" int c2s_pack_weights_winograd(const float* src, float* upk, int cin, int cout, int coutP, long stride_o,
                                         long stride_c, const int* host_tap_off, void* stream) {
    return pack_one("pack_weights_winograd", PACK_WINO, src, upk, cin, cout, coutP, 9, stride_o, stride_c, host_tap_off, stream);
}

extern "C" int c2s_pack_weights_winograd16(const float* src, float* upk, int cin, int cout, int coutP, long stride_o,
                                           long stride_c, const int* host_tap_off, void* stream) {
    return pack_one("pack_winograd16", PACK_WINO16, src, upk, cin, cout, coutP, 9, stride_o, stride_c, host_tap_off, stream);
}

extern "C" int c2s_pack_weights_s2wino(const float* src, float* upk, int cin, int cout, int coutP, long stride_o,
                                       long stride_c, const int* host_tap_off, void* stream) {
    return pack_one("pack_s2wino", PACK_S2WINO, src, upk, cin, cout, coutP, 16, stride_o, stride_c, host_tap_off, stream);
}

// kc = gy channels (the forward Cout), cs / csP = input channels of this source
extern "C" int c2s_pack_weights_s2dgrad(const float* src, float* upk, int kc, int cs, int csP, long stride_c, long stride_k,
                                        const int* host_tap_off, void* stream) {
    return pack_one("pack_s2dgrad", PACK_S2DGRAD, src, upk, kc, cs, csP, 16, stride_c, stride_k, host_tap_off, stream);
}

extern "C" size_t c2s_winograd_packed_floats(int cin, int coutP) { return pack_floats(PACK_WINO, cin, coutP, 9); }
extern "C" size_t c2s_winograd16_packed_floats(int cin, int coutP) { return pack_floats(PACK_WINO16, cin, coutP, 9); }
extern "C" size_t c2s_s2wino_packed_floats(int cin, int coutP) { return pack_floats(PACK_S2WINO, cin, coutP, 16); }
extern "C" size_t c2s_s2dgrad_packed_floats(int kc, int csP) { return pack_floats(PACK_S2DGRAD, kc, csP, 16); }

extern "C" size_t c2s_pack_job_bytes(void) { return sizeof(PackJob); }

// Fill one job record of a host-side table (the caller uploads the table once and reuses it every step)
extern "C" int c2s_pack_job_fill(void* host_record, const float* src, float* dst, int cin, int cout, int coutP, int ntaps,
                                 long stride_o, long stride_c, int winograd, const int* host_tap_off, int block_start) {
    C2S_REQUIRE(host_record, "pack_job_fill: null record");
    return pack_job_init(reinterpret_cast<PackJob*>(host_record), "pack_job_fill", winograd, src, dst, cin, cout, coutP, ntaps,
                         stride_o, stride_c, host_tap_off, block_start);
}

// blocks (of 256 threads) a job needs
extern "C" int c2s_pack_job_blocks(int cin, int coutP, int ntaps, int winograd) {
    return cdiv(pack_items(winograd, cin, coutP, ntaps), PACK_THREADS);
}

extern "C" int c2s_pack_batch(const void* device_table, int njobs, int total_blocks, void* stream) {
    C2S_REQUIRE(device_table && njobs > 0 && total_blocks > 0, "pack_batch: bad args");
    hipLaunchKernelGGL(pack_batch_kernel, dim3(total_blocks), dim3(PACK_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackJob*>(device_table), njobs);
    C2S_CHECK_LAUNCH("pack_batch");
    return C2S_OK;
}
