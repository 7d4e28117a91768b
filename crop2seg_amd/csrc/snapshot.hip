// Training-state snapshots: many live device regions <-> one contiguous device blob with a checksummed header, all on the
// stream (no allocation, no synchronisation, no read-back: legal inside a hipGraph capture).  See DESIGN.md (checkpoints) and
// include/c2s_hip.h for the blob layout.
//
// Region table (SnapJob, built on the host by c2s_snapshot_job_fill, uploaded once): region r is `bytes` (a multiple of 4, zero
// allowed) at `live`, stored at payload offset `blob_off` (a multiple of 16) and padded there with zero words to a multiple of
// 16 bytes.  The padded region is cut into spans of C2S_SNAPSHOT_SPAN_BYTES; span k of region r is virtual block
// block_start[r] + k.  The workgroups walk the virtual blocks with a grid stride and find a block's region by bisection.
// The kernels are HBM-bound copies: one 16-byte vector per lane and access where the live address is 16-byte aligned and the
// vector lies inside the region, dwords otherwise; the blob side is always 16-byte aligned.
//
// Checksums over the payload's 32-bit words w_i (padding included): s1 = sum w_i, s2 = sum (i + 1) w_i, both mod 2^64.  Every
// lane adds what it copied, the lanes meet in a wave butterfly, the waves in LDS, and each workgroup issues one 64-bit integer
// atomic per sum.  Integer addition mod 2^64 is associative and commutative, so the sums are the same bits in any order.
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int SN_THREADS = 256;
constexpr long SN_SPAN = C2S_SNAPSHOT_SPAN_BYTES;
constexpr int SN_VECS = (int)(SN_SPAN / 16 / SN_THREADS);      // 16-byte vectors per lane and span
static_assert(SN_SPAN == (long)SN_VECS * 16 * SN_THREADS, "a span is a whole number of workgroup passes");

struct SnapJob {
    void* live;
    long bytes;
    long blob_off;       // from the start of the payload
    long block_start;    // first virtual block of this region
};

struct SnapHeader {
    unsigned magic, version, nregions, zero;
    u64 payload_bytes, s1, s2;
    u64 reserved[3];
};
static_assert(sizeof(SnapHeader) == C2S_SNAPSHOT_HEADER_BYTES, "blob header layout");

struct SnapStatus {
    int ok, reason;
    u64 s1, s2;
    u64 reserved;
};
static_assert(sizeof(SnapStatus) == C2S_SNAPSHOT_STATUS_BYTES, "status block layout");

__host__ __device__ inline long snap_blocks(long bytes) { return ((bytes + 15) / 16 * 16 + SN_SPAN - 1) / SN_SPAN; }

// the region a virtual block belongs to: the largest r with block_start[r] <= vb (an empty region shares its block_start with
// the next one and is never the largest)
__device__ __forceinline__ int region_of(const SnapJob* __restrict__ jobs, int n, long vb) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].block_start <= vb) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ void sums_add(u64& s1, u64& s2, u32x4 w, u64 word) {     // `word`: payload index of w.x
    const u64 t = (u64)w.x + w.y + w.z + w.w;
    s1 += t;
    s2 += (word + 1) * t + (u64)w.y + 2 * (u64)w.z + 3 * (u64)w.w;
}

// the workgroup's two sums into dst[0], dst[1]: one atomic each
__device__ __forceinline__ void sums_commit(u64 s1, u64 s2, u64* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    __shared__ u64 sw[2][SN_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        sw[0][threadIdx.x >> 6] = s1;
        sw[1][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < SN_THREADS / 64; ++w) s += sw[threadIdx.x][w];
        atomicAdd(dst + threadIdx.x, s);
    }
}

__global__ void header_kernel(SnapHeader* __restrict__ h, unsigned nregions, u64 payload_bytes) {
    if (threadIdx.x == 0) {
        SnapHeader v = {};
        v.magic = C2S_SNAPSHOT_MAGIC;
        v.version = C2S_SNAPSHOT_VERSION;
        v.nregions = nregions;
        v.payload_bytes = payload_bytes;
        *h = v;
    }
}

// SCATTER false: live -> blob, sums into the header.  SCATTER true: blob -> live, only when the status block says ok.
template <bool SCATTER>
__global__ __launch_bounds__(SN_THREADS) void regions_kernel(const SnapJob* __restrict__ jobs, int nregions,
                                                             unsigned char* __restrict__ blob, long payload_bytes,
                                                             const SnapStatus* __restrict__ st) {
    SnapHeader* hdr = reinterpret_cast<SnapHeader*>(blob);
    if (SCATTER) {
        if (st->ok != 1 || hdr->nregions != (unsigned)nregions || hdr->payload_bytes != (u64)payload_bytes) return;
    }
    unsigned char* payload = blob + C2S_SNAPSHOT_HEADER_BYTES;
    const SnapJob last = jobs[nregions - 1];
    const long total = last.block_start + snap_blocks(last.bytes);
    u64 s1 = 0, s2 = 0;
    for (long vb = blockIdx.x; vb < total; vb += gridDim.x) {
        const int r = region_of(jobs, nregions, vb);
        if (r < 0) continue;                                    // a table that does not start at block 0
        const SnapJob j = jobs[r];
        const long padded = (j.bytes + 15) / 16 * 16;
        const long base = (vb - j.block_start) * SN_SPAN;       // byte offset of this span in the padded region
        const bool aligned = ((uintptr_t)j.live & 15) == 0;
        unsigned char* live = reinterpret_cast<unsigned char*>(j.live);
#pragma unroll
        for (int k = 0; k < SN_VECS; ++k) {
            const long b = base + ((long)k * SN_THREADS + threadIdx.x) * 16;
            if (b >= padded || j.blob_off + b + 16 > payload_bytes) continue;     // never past the region or the blob
            u32x4* bp = reinterpret_cast<u32x4*>(payload + j.blob_off + b);
            const bool whole = b + 16 <= j.bytes;
            if (!SCATTER) {
                u32x4 w = {0u, 0u, 0u, 0u};
                if (whole && aligned) {
                    w = *reinterpret_cast<const u32x4*>(live + b);
                } else {
                    const unsigned* lp = reinterpret_cast<const unsigned*>(live + b);
                    if (b < j.bytes) w.x = lp[0];
                    if (b + 4 < j.bytes) w.y = lp[1];
                    if (b + 8 < j.bytes) w.z = lp[2];
                    if (b + 12 < j.bytes) w.w = lp[3];
                }
                *bp = w;                                        // padding words are written as 0
                sums_add(s1, s2, w, (u64)((j.blob_off + b) >> 2));
            } else {
                const u32x4 w = *bp;
                if (whole && aligned) {
                    *reinterpret_cast<u32x4*>(live + b) = w;
                } else {
                    unsigned* lp = reinterpret_cast<unsigned*>(live + b);
                    if (b < j.bytes) lp[0] = w.x;
                    if (b + 4 < j.bytes) lp[1] = w.y;
                    if (b + 8 < j.bytes) lp[2] = w.z;
                    if (b + 12 < j.bytes) lp[3] = w.w;
                }
            }
        }
    }
    if (!SCATTER) sums_commit(s1, s2, &hdr->s1);
}

__global__ void status_clear_kernel(SnapStatus* __restrict__ st) {
    if (threadIdx.x == 0) {
        SnapStatus v = {};
        *st = v;
    }
}

// both sums of the payload into the status block
__global__ __launch_bounds__(SN_THREADS) void sums_kernel(const unsigned char* __restrict__ blob, long payload_bytes,
                                                          SnapStatus* __restrict__ st) {
    const u32x4* p = reinterpret_cast<const u32x4*>(blob + C2S_SNAPSHOT_HEADER_BYTES);
    const long nvec = payload_bytes / 16;
    u64 s1 = 0, s2 = 0;
    for (long v = blockIdx.x * (long)SN_THREADS + threadIdx.x; v < nvec; v += (long)gridDim.x * SN_THREADS)
        sums_add(s1, s2, p[v], (u64)v * 4);
    sums_commit(s1, s2, &st->s1);
}

__global__ void verdict_kernel(const SnapHeader* __restrict__ h, long payload_bytes, unsigned nregions,
                               SnapStatus* __restrict__ st) {
    if (threadIdx.x != 0) return;
    int reason = 0;
    if (h->magic != C2S_SNAPSHOT_MAGIC) reason = 1;
    else if (h->version != C2S_SNAPSHOT_VERSION) reason = 2;
    else if (h->nregions != nregions) reason = 3;
    else if (h->payload_bytes != (u64)payload_bytes) reason = 4;
    else if (h->s1 != st->s1 || h->s2 != st->s2) reason = 5;
    st->reason = reason;
    st->ok = reason == 0 ? 1 : 0;
}

int grid_blocks(long vblocks) {
    return (int)(vblocks < 1 ? 1 : (vblocks > C2S_SNAPSHOT_MAX_BLOCKS ? C2S_SNAPSHOT_MAX_BLOCKS : vblocks));
}

}  // namespace

extern "C" size_t c2s_snapshot_job_bytes(void) { return sizeof(SnapJob); }

extern "C" long c2s_snapshot_job_blocks(long bytes) { return bytes < 0 ? -1 : snap_blocks(bytes); }

extern "C" int c2s_snapshot_job_fill(void* host_record, const void* live, long bytes, long blob_offset, long block_start) {
    C2S_REQUIRE(host_record, "snapshot_job_fill: null record");
    C2S_REQUIRE(bytes >= 0 && bytes % 4 == 0, "snapshot_job_fill: a region of %ld bytes, a multiple of 4 is needed", bytes);
    C2S_REQUIRE(live || bytes == 0, "snapshot_job_fill: null region of %ld bytes", bytes);
    C2S_REQUIRE((uintptr_t)live % 4 == 0, "snapshot_job_fill: region not 4-byte aligned");
    C2S_REQUIRE(blob_offset >= 0 && blob_offset % 16 == 0, "snapshot_job_fill: blob offset %ld, a multiple of 16 is needed",
                blob_offset);
    C2S_REQUIRE(block_start >= 0, "snapshot_job_fill: negative block_start");
    SnapJob* j = reinterpret_cast<SnapJob*>(host_record);
    j->live = const_cast<void*>(live);
    j->bytes = bytes;
    j->blob_off = blob_offset;
    j->block_start = block_start;
    return C2S_OK;
}

static int blob_args(const char* who, const void* blob, long blob_bytes) {
    C2S_REQUIRE(blob && (uintptr_t)blob % 16 == 0, "%s: the blob must be 16-byte aligned", who);
    C2S_REQUIRE(blob_bytes >= C2S_SNAPSHOT_HEADER_BYTES && blob_bytes % 16 == 0,
                "%s: a blob of %ld bytes (the header's %d and a multiple of 16 are needed)", who, blob_bytes,
                C2S_SNAPSHOT_HEADER_BYTES);
    return C2S_OK;
}

extern "C" int c2s_snapshot_gather(const void* device_table, int nregions, void* blob, long blob_bytes, void* stream) {
    C2S_REQUIRE(device_table && nregions > 0, "snapshot_gather: bad args");
    C2S_REQUIRE((uintptr_t)device_table % 8 == 0, "snapshot_gather: table not 8-byte aligned");
    const int rc = blob_args("snapshot_gather", blob, blob_bytes);
    if (rc != C2S_OK) return rc;
    const long payload = blob_bytes - C2S_SNAPSHOT_HEADER_BYTES;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(header_kernel, dim3(1), dim3(64), 0, st, (SnapHeader*)blob, (unsigned)nregions, (u64)payload);
    C2S_CHECK_LAUNCH("snapshot_header");
    // virtual blocks <= payload / span + one ragged span per region
    hipLaunchKernelGGL(regions_kernel<false>, dim3(grid_blocks(payload / SN_SPAN + nregions)), dim3(SN_THREADS), 0, st,
                       (const SnapJob*)device_table, nregions, (unsigned char*)blob, payload, (const SnapStatus*)nullptr);
    C2S_CHECK_LAUNCH("snapshot_gather");
    return C2S_OK;
}

extern "C" int c2s_snapshot_verify(const void* blob, long blob_bytes, int nregions, void* status, void* stream) {
    C2S_REQUIRE(status && (uintptr_t)status % 8 == 0 && nregions > 0, "snapshot_verify: bad args");
    const int rc = blob_args("snapshot_verify", blob, blob_bytes);
    if (rc != C2S_OK) return rc;
    const long payload = blob_bytes - C2S_SNAPSHOT_HEADER_BYTES;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(status_clear_kernel, dim3(1), dim3(64), 0, st, (SnapStatus*)status);
    C2S_CHECK_LAUNCH("snapshot_status_clear");
    hipLaunchKernelGGL(sums_kernel, dim3(grid_blocks((payload / 16 + SN_THREADS - 1) / SN_THREADS)), dim3(SN_THREADS), 0, st,
                       (const unsigned char*)blob, payload, (SnapStatus*)status);
    C2S_CHECK_LAUNCH("snapshot_sums");
    hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(64), 0, st, (const SnapHeader*)blob, payload, (unsigned)nregions,
                       (SnapStatus*)status);
    C2S_CHECK_LAUNCH("snapshot_verdict");
    return C2S_OK;
}

extern "C" int c2s_snapshot_scatter(const void* device_table, int nregions, const void* blob, long blob_bytes,
                                    const void* status, void* stream) {
    C2S_REQUIRE(device_table && nregions > 0 && status, "snapshot_scatter: bad args");
    C2S_REQUIRE((uintptr_t)device_table % 8 == 0 && (uintptr_t)status % 8 == 0, "snapshot_scatter: table / status not 8-byte aligned");
    const int rc = blob_args("snapshot_scatter", blob, blob_bytes);
    if (rc != C2S_OK) return rc;
    const long payload = blob_bytes - C2S_SNAPSHOT_HEADER_BYTES;
    hipLaunchKernelGGL(regions_kernel<true>, dim3(grid_blocks(payload / SN_SPAN + nregions)), dim3(SN_THREADS), 0,
                       (hipStream_t)stream, (const SnapJob*)device_table, nregions,
                       (unsigned char*)const_cast<void*>(blob), payload, (const SnapStatus*)status);
    C2S_CHECK_LAUNCH("snapshot_scatter");
    return C2S_OK;
}
