// Attention dropout of the L-TAE kernels (tae.py:837), shared by every family (ltae.hip, ltae_long.hip) so that a given
// (seed, head, pixel, t) gets the same decision whichever family runs.  Explicit keep mask [16,P,T] (tests) or a
// counter-based RNG: ONE 32-bit avalanche hash per pair of time steps (2u, 2u+1) of a (head, pixel) row, 16 bits per
// element -- drop probability round(p * 2^16) / 2^16 with the matching scale, so E[keep * scale] = 1 exactly.  (Two full
// hashes per element cost 4 quarter-rate v_mul_lo_u32 each: 6.6k of the 12k cycles the dropout + store phase of a 16-pixel
// tile took.)
#pragma once
#include "common.h"

struct DropCtx {
    uint32_t key, thr;
    float inv;
    int half_t;
};
__device__ __forceinline__ DropCtx drop_ctx_of(uint64_t seed0, const uint64_t* seed_dev, float drop_p, int T) {
    DropCtx d;
    const uint64_t seed = seed0 + (seed_dev != nullptr ? *seed_dev * 0x9E3779B97F4A7C15ull : 0ull);
    d.key = c2s_hash32((uint32_t)seed ^ c2s_hash32((uint32_t)(seed >> 32) + 0x9E3779B9u));
    d.thr = (uint32_t)(drop_p * 65536.f + 0.5f);
    d.inv = 65536.f / (65536.f - (float)d.thr);
    d.half_t = (T + 1) >> 1;
    return d;
}
__device__ __forceinline__ uint32_t drop_bits(const DropCtx& d, long row, int u) {
    const uint64_t i2 = (uint64_t)row * (uint64_t)d.half_t + (uint64_t)u;
    return c2s_hash32((uint32_t)i2 ^ d.key ^ (uint32_t)(i2 >> 32) * 0x85EBCA6Bu);
}
__device__ __forceinline__ float drop_pick(const DropCtx& d, uint32_t bits, int t) {
    const uint32_t u16 = (t & 1) ? bits >> 16 : bits & 0xffffu;
    return u16 >= d.thr ? d.inv : 0.f;
}
