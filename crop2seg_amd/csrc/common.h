// Shared device/host helpers for libc2s_hip.so (gfx950 only: wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/c2s_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// the same four floats at an address that is only float-aligned (a row of HW % 4 != 0 floats starts anywhere): global
// memory takes a 16-byte access at any 4-byte boundary, but the type must say so -- a plain f32x4 promises 16
typedef f32x4 f32x4u __attribute__((aligned(4)));

void c2s_set_error(const char* fmt, ...);

// Per-device one-time set-up (misc.hip).  Every source file registers a hook that raises the dynamic-LDS limit of its
// kernels; c2s_init(device) / c2s_ensure_init() run all hooks once per device under a mutex and cache the device's CU
// count.  Entry points call c2s_ensure_init() (one thread-local hipGetDevice + an atomic load when already done), so a
// caller that ran c2s_init() before capturing a hipGraph never triggers set-up work inside the capture.
typedef void (*c2s_init_hook)(void);
struct C2sInitRegistrar {
    explicit C2sInitRegistrar(c2s_init_hook hook);
};
void c2s_ensure_init();
int c2s_cus();   // compute units of the current device (256 when no device is present: CPU-side argument checks)
#define C2S_RAISE_LDS(kernel) \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)

#define C2S_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            c2s_set_error(__VA_ARGS__);   \
            return C2S_EINVAL;            \
        }                                 \
    } while (0)

#define C2S_CHECK_LAUNCH(name)                                              \
    do {                                                                    \
        hipError_t e__ = hipGetLastError();                                 \
        if (e__ != hipSuccess) {                                            \
            c2s_set_error("%s: %s", name, hipGetErrorString(e__));          \
            return C2S_ELAUNCH;                                             \
        }                                                                   \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
// A launch with one thread per item and no grid-stride loop: gridDim.x x blockDim.x, the work-items of ONE grid dimension, must
// fit 32 bits.  HIP takes a larger one without an error and does not run all of it (measured on an MI355X: the items past 2^32
// were never written).  The limit is per dimension: the product over x, y and z may be far larger (the folded depthwise
// launch), and folding over y / z does not lift the limit of x.  `total` = the work-items along x.
#define C2S_REQUIRE_ITEMS(total, block, what)                                                              \
    C2S_REQUIRE(((long)(total) + (block) - 1) / (block) * (long)(block) < (1L << 32),                      \
                what ": %ld work-items in one launch, the limit is 2^32 - 1", (long)(total))
// blocks of 256 threads for a grid-stride loop over n elements, at most `cap`.  No default: a cap is behaviour (the number
// of block partials fixes the bits of a loss), so every call site states its own.
static inline int grid_for(long n, int cap) {
    long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// One element of torch.optim.Adam (train.py:454, torch defaults): shared by adam_kernel (misc.hip) and adam_slots_kernel
// (guard.hip) so that the two cannot drift apart.  bc1 = 1 - b1^step, bc2s = sqrt(1 - b2^step) (adam_bias).
__device__ __forceinline__ void adam_bias(float b1, float b2, int st, float& bc1, float& bc2s) {
    bc1 = 1.f - powf(b1, (float)st);
    bc2s = sqrtf(1.f - powf(b2, (float)st));
}
// The statements behind gg, the gradient Adam sees, are a macro so that adam_element keeps its text and adam_element_wd
// (coupled weight decay folded into gg: adam_slots_hp_kernel, guard.hip) states no arithmetic of its own.
#define C2S_ADAM_ELEMENT_FROM_GG                                  \
    const float mm = b1 * m[i] + (1.f - b1) * gg;                 \
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;            \
    m[i] = mm; v[i] = vv;                                         \
    const float denom = sqrtf(vv) / bc2s + eps;                   \
    p[i] -= (lr / bc1) * (mm / denom);
__device__ __forceinline__ void adam_element(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, long i, float lr, float b1, float b2, float eps,
                                             float bc1, float bc2s, float gscale) {
    const float gg = g[i] * gscale;
    C2S_ADAM_ELEMENT_FROM_GG
}
// torch.optim.Adam(weight_decay=wd): the decay joins the scaled (clipped) gradient, gg = g gscale + wd p
__device__ __forceinline__ void adam_element_wd(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, long i, float lr, float b1, float b2, float eps,
                                                float bc1, float bc2s, float gscale, float wd) {
    float gg = g[i] * gscale;
    gg = gg + wd * p[i];
    C2S_ADAM_ELEMENT_FROM_GG
}
// taps of the largest packed kernel (the 6x6 stride-2 convolutions): tap tables of the weight packs and slice sums
constexpr int C2S_MAX_TAPS = 36;
// classes of the kernels that keep a per-class table on chip (the reference uses 15; PASTIS 20): the confusion matrices of
// metrics.hip, the class mask and the registers of loss.hip, the votes of parcels.hip
constexpr int C2S_MAX_CLASSES = 32;

// Packed Winograd layouts: written by pack.hip, read by the convolution kernels named
constexpr int WN_CK = 8;                            // conv_winograd.hip: input channels per chunk
constexpr int WN_USLAB = 16 * WN_CK * 64;           // floats of one U chunk
constexpr int W16_CK = 8;                           // conv_winograd16.hip: input channels per chunk
constexpr int W16_UP = 16;                          // floats per (c, o): the 16 points, stored [c][xi 4][o 64][nu 4]
constexpr int S2_UP = 12;                           // conv_s2wino.hip: floats per (c, parity, o): 9 points + 3 zeros
constexpr int D2_UP = 12;                           // conv_s2dgrad.hip: floats per (k, parity, c): 9 points + 3 zeros

// XCD-aware order: workgroups go to the 8 XCDs round-robin in launch order, so item i of n is renumbered such that XCD k gets
// the k-th contiguous eighth of the items (neighbours, which share halo rows or cache lines, then sit behind the same L2).
// The identity where n does not divide by 8.  A macro, in the caller's index type (int or unsigned): as an inline function
// the same expression came out with the other branch polarity in the persistent kernels, whose assembly is pinned.
#define C2S_XCD_ORDER(i, n) (((n) & 7) == 0 ? ((i) & 7) * ((n) >> 3) + ((i) >> 3) : (i))

__device__ __forceinline__ int reflect_idx(int i, int n) {
    // single reflection (pad < n): -1 -> 1, n -> n-2
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// counter-based RNG: two rounds of a 32-bit avalanche hash (multiply / xor-shift) over (index, key): uniform in [0,1).
// 14 integer VALU ops per draw (a 64-bit splitmix finaliser costs ~30 on this ISA: no 64-bit multiplier) -- the L-TAE
// kernels draw one number per attention element, 976 per pixel at T = 61.
__device__ __forceinline__ uint32_t c2s_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float c2s_uniform(uint64_t seed, uint64_t idx) {
    uint32_t h = c2s_hash32((uint32_t)idx ^ (uint32_t)seed);
    h = c2s_hash32(h ^ (uint32_t)(idx >> 32) * 0x9E3779B9u ^ (uint32_t)(seed >> 32));
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}
