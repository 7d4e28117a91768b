// Union-find over the pixels of a raster batch: the index arithmetic, find, link and the iteration cap of the connected-
// component labelling in parcels.hip, kept as __host__ __device__ functions so that a stand-alone host program can drive
// them sequentially under a sanitizer (tools/parcel_uf_check.cpp: bounds and termination, not the atomics).
//
// parent[] holds one int per pixel of the batch, indexed by the GLOBAL pixel index i = (b * H + y) * W + x.
// Invariants: parent[i] <= i, parent[i] lies in the image of i, and parent[i] is in the 4-connected component of i.  A root
// has parent[r] == r; the root of a finished component is its smallest pixel index.  Links only ever lower a parent
// (atomicMin), so a value read a little late is still an ancestor: following it ends at the same root.
#pragma once

#if defined(__HIPCC__)
#define PUF_HD __host__ __device__ __forceinline__
#else
#define PUF_HD inline
#endif

// the two neighbours a pixel is united with (left and upper); the other two are covered from the other side.  Nothing
// connects the last column of a row to the first of the next, nor the last row of an image to the first of the next.
PUF_HD bool puf_has_left(int i, int W) { return i % W > 0; }
PUF_HD bool puf_has_up(int i, int H, int W) { return (i / W) % H > 0; }

PUF_HD int puf_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // never a value kept in a register
#else
    return *p;
#endif
}

// parent[b] = min(parent[b], a); returns what was there
PUF_HD int puf_min(int* p, int a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, a);
#else
    const int old = *p;
    if (a < old) *p = a;
    return old;
#endif
}

// The root above i, or -1 after more than `cap` steps.  Every step lowers the index, so H * W steps always suffice: the cap
// is hit only when parent[] is damaged, and then the walk ends instead of spinning.
PUF_HD int puf_find(const int* parent, int i, int cap) {
    for (int s = 0; s <= cap; ++s) {
        const int p = puf_load(parent + i);
        if (p == i) return i;
        i = p;
    }
    return -1;
}

// Unites the sets of a and b: the larger root goes under the smaller.  When another link got to the larger root first
// (the atomicMin does not return the root itself), the work goes on from what that root points to now: the larger of
// the two indices falls with every retry, so `cap` retries always suffice.  false: a cap was hit.
PUF_HD bool puf_unite(int* parent, int a, int b, int cap) {
    for (int s = 0; s <= cap; ++s) {
        a = puf_find(parent, a, cap);
        b = puf_find(parent, b, cap);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = puf_min(parent + b, a);
        if (old == b) return true;
        b = old;
    }
    return false;
}

// pass 2 of the labelling for pixel i of a B x H x W mask batch
PUF_HD bool puf_unite_pixel(int* parent, const unsigned char* mask, int i, int H, int W, int cap) {
    bool ok = true;
    if (puf_has_left(i, W) && mask[i - 1]) ok = puf_unite(parent, i, i - 1, cap) && ok;
    if (puf_has_up(i, H, W) && mask[i - W]) ok = puf_unite(parent, i, i - W, cap) && ok;
    return ok;
}
