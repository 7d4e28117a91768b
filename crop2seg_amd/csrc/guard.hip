// Guarded optimiser step: the gradient norm of the trainable slots of the flat gradient buffer, the clip / skip decision,
// Adam over all slots in one launch and the roll-back of the model's floating-point buffers, all on the stream (no
// allocation, no synchronisation, no read-back: legal inside a hipGraph capture).  See DESIGN.md (train step).
//
// Slot table: long[nslots][2] = (offset, length) in floats, offsets ascending, slots disjoint; whatever lies between the end of
// a slot and the next offset is padding and is neither read nor written.  mask: int[nslots], non-zero = trainable.
// All kernels are HBM- or latency-bound passes over at most a few MB (4.3 MB for U-TAE): one dword per lane and access,
// coalesced, as adam_kernel (misc.hip) does it.
//
// Also here, on the same slot table: the learning-rate schedule (a device table read at a device position, c2s_lr_advance) and
// Adam with a per-slot rate multiplier and weight decay (c2s_adam_slots_hp), so that a captured step replays a schedule.
#include <limits.h>
#include "common.h"

namespace {

constexpr int GD_CHUNK = 2048;       // floats one workgroup pass covers: 256 lanes x 8
constexpr int GD_PARTIALS = 256;     // workgroups of the sum-of-squares pass = doubles of its workspace

// the status block (32 bytes): c2s_hip.h documents the layout
struct GuardStatus {
    double sumsq;
    int ok;
    float scale;
    float norm;
    float coef;
    int reserved[2];
};
static_assert(sizeof(GuardStatus) == C2S_GUARD_STATUS_BYTES, "status block layout");

// the slot an element lies in or behind: the largest s with offset[s] <= i, -1 in front of the first slot
__device__ __forceinline__ int slot_search(const long* __restrict__ slots, int nslots, long i) {
    int lo = 0, hi = nslots;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (slots[2 * mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// Walks the slot table forward with the element index: after seek(i), `s` is the slot i lies in or behind, and i is an
// element of a trainable slot iff live(i).
struct SlotCursor {
    const long* __restrict__ slots;
    const int* __restrict__ mask;
    int nslots, s;
    long end, next;     // end of slot s (clamped to the next offset and to `total`); offset of slot s + 1
    bool on;
    __device__ __forceinline__ void load(long total) {
        next = s + 1 < nslots ? slots[2 * (s + 1)] : LONG_MAX;
        end = 0;
        on = false;
        if (s >= 0) {
            end = slots[2 * s] + slots[2 * s + 1];
            end = end < next ? end : next;
            end = end < total ? end : total;
            on = mask[s] != 0;
        }
    }
    __device__ __forceinline__ void start(const long* sl, const int* mk, int n, long i, long total) {
        slots = sl; mask = mk; nslots = n;
        s = slot_search(sl, n, i);
        load(total);
    }
    __device__ __forceinline__ void seek(long i, long total) {
        if (i < next) return;
        do {
            ++s;
            next = s + 1 < nslots ? slots[2 * (s + 1)] : LONG_MAX;
        } while (i >= next);
        load(total);
    }
    __device__ __forceinline__ bool live(long i) const { return on && i < end; }
};

// ---------------------------------------------------------------- sum of squares (fp64, fixed order)
// Workgroup b reduces the chunks [b * cpw, (b + 1) * cpw): every lane adds its elements in index order, the lanes of a wave
// meet in a shuffle butterfly, the four waves through LDS in wave order.  One partial per workgroup.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const long* __restrict__ slots,
                                                         const int* __restrict__ mask, int nslots, long total, long nchunks,
                                                         long cpw, double* __restrict__ partials) {
    const long c0 = blockIdx.x * cpw;
    const long c1 = c0 + cpw < nchunks ? c0 + cpw : nchunks;
    SlotCursor cur;
    cur.start(slots, mask, nslots, c0 * GD_CHUNK, total);
    double acc = 0.0;
    for (long c = c0; c < c1; ++c) {
        for (int k = 0; k < GD_CHUNK / 256; ++k) {
            const long i = c * GD_CHUNK + k * 256 + threadIdx.x;
            if (i >= total) break;
            cur.seek(i, total);
            if (cur.live(i)) {                   // frozen slots and padding are not read
                const double x = (double)g[i];
                acc += x * x;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double sw[4];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// the partials in index order
__global__ __launch_bounds__(256) void grad_sumsq_final_kernel(const double* __restrict__ partials, int n,
                                                               GuardStatus* __restrict__ st) {
    __shared__ double sp[GD_PARTIALS];
    if ((int)threadIdx.x < n) sp[threadIdx.x] = partials[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += sp[i];
        st->sumsq = s;
    }
}

// ---------------------------------------------------------------- the decision (torch.nn.utils.clip_grad_norm_, norm_type 2)
__global__ __launch_bounds__(256) void step_decide_kernel(GuardStatus* __restrict__ st, float max_grad_norm, float grad_scale,
                                                          int skip_nonfinite, const int* __restrict__ mask,
                                                          int* __restrict__ slot_steps, int nslots,
                                                          int* __restrict__ skip_count) {
    const double ss = st->sumsq;
    const bool ok = !skip_nonfinite || (ss - ss == 0.0);        // finite: neither inf nor NaN
    if (ok)
        for (int s = threadIdx.x; s < nslots; s += blockDim.x)
            if (mask[s] != 0) slot_steps[s] += 1;
    if (threadIdx.x == 0) {
        const double norm = (double)grad_scale * sqrt(ss);      // of the gradient Adam sees: after the 1/world scale
        double coef = 1.0;
        if (max_grad_norm > 0.f) {
            coef = (double)max_grad_norm / (norm + 1e-6);
            coef = coef < 1.0 ? coef : 1.0;                     // a NaN norm leaves 1: the step is applied as it is
        }
        st->ok = ok ? 1 : 0;
        st->scale = (float)((double)grad_scale * coef);
        st->norm = (float)norm;
        st->coef = (float)coef;
        if (!ok) skip_count[0] += 1;
    }
}

// ---------------------------------------------------------------- Adam over all slots (train.py:454)
__global__ __launch_bounds__(256) void adam_slots_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         const long* __restrict__ slots, const int* __restrict__ mask,
                                                         const int* __restrict__ slot_steps, int nslots, long total, float lr,
                                                         float b1, float b2, float eps, const GuardStatus* __restrict__ st) {
    if (st->ok == 0) return;                                    // a skipped step writes nothing
    const float gscale = st->scale;
    const long base = (long)blockIdx.x * GD_CHUNK;
    SlotCursor cur;
    cur.start(slots, mask, nslots, base, total);
    int bs = -1;                                                // the slot bc1 / bc2s belong to
    float bc1 = 1.f, bc2s = 1.f;
    for (int k = 0; k < GD_CHUNK / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i >= total) break;
        cur.seek(i, total);
        if (!cur.live(i)) continue;
        if (cur.s != bs) {
            bs = cur.s;
            adam_bias(b1, b2, slot_steps[bs], bc1, bc2s);       // the slot's own step count
        }
        adam_element(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2s, gscale);
    }
}

// ---------------------------------------------------------------- learning-rate schedule and per-slot hyper-parameters
// the schedule state block (16 bytes): c2s_hip.h documents the layout
struct SchedState {
    int t;
    float scale;
    float lr_now;
    int zero;
};
static_assert(sizeof(SchedState) == C2S_SCHED_STATE_BYTES, "schedule state block layout");

// One workgroup.  Applied step: lr_now = table[min(t, n - 1)] * scale (in double, rounded once), t += 1; a skipped step leaves the
// block alone.  Without a status block nobody has counted the step yet: the trainable slots' counts advance here.
__global__ __launch_bounds__(256) void lr_advance_kernel(SchedState* __restrict__ sc, const float* __restrict__ table, int n,
                                                         const int* __restrict__ mask, int* __restrict__ slot_steps, int nslots,
                                                         const GuardStatus* __restrict__ st) {
    if (st != nullptr) {
        if (st->ok == 0) return;
    } else {
        for (int s = threadIdx.x; s < nslots; s += blockDim.x)
            if (mask[s] != 0) slot_steps[s] += 1;
    }
    if (threadIdx.x == 0) {
        const int t = sc->t;
        int k = t < n - 1 ? t : n - 1;
        k = k < 0 ? 0 : k;
        sc->lr_now = (float)((double)table[k] * (double)sc->scale);
        sc->t = t < INT_MAX ? t + 1 : t;
    }
}

// adam_slots_kernel with the rate from the schedule block and (lr multiplier, weight decay) per slot: hp is float[nslots][2],
// read where the bias corrections are read.  A slot without decay runs adam_element as adam_slots_kernel does.
__global__ __launch_bounds__(256) void adam_slots_hp_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            const long* __restrict__ slots, const int* __restrict__ mask,
                                                            const int* __restrict__ slot_steps, const float* __restrict__ hp,
                                                            int nslots, long total, const SchedState* __restrict__ sc, float b1,
                                                            float b2, float eps, int decoupled, float grad_scale,
                                                            const GuardStatus* __restrict__ st) {
    float gscale = grad_scale;
    if (st != nullptr) {
        if (st->ok == 0) return;                                // a skipped step writes nothing
        gscale = st->scale;
    }
    const float lr_now = sc->lr_now;
    const long base = (long)blockIdx.x * GD_CHUNK;
    SlotCursor cur;
    cur.start(slots, mask, nslots, base, total);
    int bs = -1;                                                // the slot bc1 / bc2s / lr / wd belong to
    float bc1 = 1.f, bc2s = 1.f, lr = 0.f, wd = 0.f;
    for (int k = 0; k < GD_CHUNK / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i >= total) break;
        cur.seek(i, total);
        if (!cur.live(i)) continue;
        if (cur.s != bs) {
            bs = cur.s;
            adam_bias(b1, b2, slot_steps[bs], bc1, bc2s);
            lr = lr_now * hp[2 * bs];
            wd = hp[2 * bs + 1];
        }
        if (wd == 0.f) {
            adam_element(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2s, gscale);
        } else if (decoupled != 0) {                            // torch.optim.AdamW: p *= 1 - lr wd, then the step
            p[i] = p[i] * (1.f - lr * wd);
            adam_element(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2s, gscale);
        } else {                                                // torch.optim.Adam(weight_decay=): g += wd p, after the clip
            adam_element_wd(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2s, gscale, wd);
        }
    }
}

__global__ void restore_if_skipped_kernel(float* __restrict__ dst, const float* __restrict__ saved, long n,
                                          const GuardStatus* __restrict__ st) {
    if (st->ok != 0) return;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = saved[i];
}

}  // namespace

extern "C" size_t c2s_grad_sumsq_workspace_doubles(void) { return GD_PARTIALS; }

extern "C" int c2s_grad_sumsq(const float* g, const long* slots, const int* mask, int nslots, long total, double* workspace,
                              size_t ws_doubles, void* status, void* stream) {
    C2S_REQUIRE(g && slots && mask && workspace && status && nslots > 0 && total > 0, "grad_sumsq: bad args");
    C2S_REQUIRE(ws_doubles >= (size_t)GD_PARTIALS, "grad_sumsq: workspace of %zu doubles, %d needed", ws_doubles, GD_PARTIALS);
    C2S_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)status % 8 == 0, "grad_sumsq: workspace / status not 8-byte aligned");
    const long nchunks = (total + GD_CHUNK - 1) / GD_CHUNK;
    const long cpw = (nchunks + GD_PARTIALS - 1) / GD_PARTIALS;
    const int blocks = (int)((nchunks + cpw - 1) / cpw);        // <= GD_PARTIALS, a function of `total` alone
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(256), 0, st, g, slots, mask, nslots, total, nchunks, cpw, workspace);
    C2S_CHECK_LAUNCH("grad_sumsq");
    hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, st, workspace, blocks, (GuardStatus*)status);
    C2S_CHECK_LAUNCH("grad_sumsq_final");
    return C2S_OK;
}

extern "C" int c2s_step_decide(void* status, float max_grad_norm, float grad_scale, int skip_nonfinite, const int* mask,
                               int* slot_steps, int nslots, int* skip_count, void* stream) {
    C2S_REQUIRE(status && mask && slot_steps && skip_count && nslots > 0, "step_decide: bad args");
    C2S_REQUIRE((uintptr_t)status % 8 == 0, "step_decide: status not 8-byte aligned");
    C2S_REQUIRE(grad_scale > 0.f && !(max_grad_norm != max_grad_norm), "step_decide: grad_scale %g, max_grad_norm %g",
                (double)grad_scale, (double)max_grad_norm);
    hipLaunchKernelGGL(step_decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (GuardStatus*)status, max_grad_norm,
                       grad_scale, skip_nonfinite, mask, slot_steps, nslots, skip_count);
    C2S_CHECK_LAUNCH("step_decide");
    return C2S_OK;
}

extern "C" int c2s_adam_slots(float* p, const float* g, float* m, float* v, const long* slots, const int* mask,
                              const int* slot_steps, int nslots, long total, float lr, float b1, float b2, float eps,
                              const void* status, void* stream) {
    C2S_REQUIRE(p && g && m && v && slots && mask && slot_steps && status && nslots > 0 && total > 0, "adam_slots: bad args");
    const long nchunks = (total + GD_CHUNK - 1) / GD_CHUNK;
    C2S_REQUIRE(nchunks <= INT_MAX, "adam_slots: %ld floats are more than one grid covers", total);
    hipLaunchKernelGGL(adam_slots_kernel, dim3((int)nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, slots, mask,
                       slot_steps, nslots, total, lr, b1, b2, eps, (const GuardStatus*)status);
    C2S_CHECK_LAUNCH("adam_slots");
    return C2S_OK;
}

extern "C" int c2s_lr_advance(void* sched, const float* table, int n, const int* mask, int* slot_steps, int nslots,
                              const void* status, void* stream) {
    C2S_REQUIRE(sched && table && mask && slot_steps && n >= 1 && nslots > 0, "lr_advance: bad args");
    C2S_REQUIRE((uintptr_t)sched % 8 == 0 && (uintptr_t)status % 8 == 0, "lr_advance: sched / status not 8-byte aligned");
    hipLaunchKernelGGL(lr_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (SchedState*)sched, table, n, mask,
                       slot_steps, nslots, (const GuardStatus*)status);
    C2S_CHECK_LAUNCH("lr_advance");
    return C2S_OK;
}

extern "C" int c2s_adam_slots_hp(float* p, const float* g, float* m, float* v, const long* slots, const int* mask,
                                 const int* slot_steps, const float* hp, int nslots, long total, const void* sched, float b1,
                                 float b2, float eps, int decoupled, float grad_scale, const void* status, void* stream) {
    C2S_REQUIRE(p && g && m && v && slots && mask && slot_steps && hp && sched && nslots > 0 && total > 0,
                "adam_slots_hp: bad args");
    C2S_REQUIRE((uintptr_t)sched % 8 == 0 && (uintptr_t)status % 8 == 0, "adam_slots_hp: sched / status not 8-byte aligned");
    C2S_REQUIRE(status != nullptr || grad_scale > 0.f, "adam_slots_hp: grad_scale %g", (double)grad_scale);
    const long nchunks = (total + GD_CHUNK - 1) / GD_CHUNK;
    C2S_REQUIRE(nchunks <= INT_MAX, "adam_slots_hp: %ld floats are more than one grid covers", total);
    hipLaunchKernelGGL(adam_slots_hp_kernel, dim3((int)nchunks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, slots, mask,
                       slot_steps, hp, nslots, total, (const SchedState*)sched, b1, b2, eps, decoupled, grad_scale,
                       (const GuardStatus*)status);
    C2S_CHECK_LAUNCH("adam_slots_hp");
    return C2S_OK;
}

extern "C" int c2s_restore_if_skipped(float* dst, const float* saved, long n, const void* status, void* stream) {
    C2S_REQUIRE(dst && saved && status && n >= 0, "restore_if_skipped: bad args");
    if (n == 0) return C2S_OK;
    const long b = (n + 255) / 256;
    hipLaunchKernelGGL(restore_if_skipped_kernel, dim3((int)(b > 1024 ? 1024 : b)), dim3(256), 0, (hipStream_t)stream, dst,
                       saved, n, (const GuardStatus*)status);
    C2S_CHECK_LAUNCH("restore_if_skipped");
    return C2S_OK;
}
