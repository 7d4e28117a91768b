// Time-chunked L-TAE family (ltae_long.hip): any T.  Launched by c2s_ltae_attn_fwd_ws / c2s_ltae_attn_bwd (ltae.hip), which
// own the argument checks, the workspace layout and the fixed-order reductions of the backward's per-tile partials.
#pragma once
#include "common.h"

constexpr int LONG_PX = 64;      // pixels per tile: lane = pixel, every access one 256-byte row segment

struct LtaeLongArgs {
    // forward inputs / outputs (attn_pre doubles as the scratch of the raw scores)
    const float* x; const float* gamma; const float* beta; const float* U; const float* s0;
    const float* Wc; const float* bc; const float* pe; const int* valid; const float* keep;
    float* attn; float* attn_pre; float* emb; float* stats;
    // backward
    const float* attn_in; const float* attn_pre_in; const float* stats_in; const float* g_emb; const float* g_attn;
    float* gx; float* GS; float* Z; float* part_s0; float* part_bc; float* part_gb; float* part_U;
    float* M;        // [P][16][2]  GroupNorm-backward means m1, m2
    float* ASG;      // [2][16][P]  sum_t attn, sum_t gs
    int B, T, C, HW;
    float eps, drop_p;
    uint64_t seed;
    const uint64_t* seed_dev;
};

inline int ltae_long_tiles(int B, int HW) { return B * ((HW + LONG_PX - 1) / LONG_PX); }
int ltae_long_fwd(const LtaeLongArgs& a, hipStream_t st);
int ltae_long_bwd(const LtaeLongArgs& a, hipStream_t st);
