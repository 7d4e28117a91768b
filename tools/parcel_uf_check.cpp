// Development check of crop2seg_amd/csrc/parcels_uf.h on the host: drives the union-find of the component labelling
// sequentially (pixel by pixel, in raster order and in reverse) over the mask patterns of tests/test_parcel_gpu.py and
// compares the roots with a flood fill.  It proves bounds and termination of the index arithmetic, find, link and the
// cap -- not the atomics, which only a GPU run exercises.  Not part of the test suite; build and run by hand:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/parcel_uf_check.cpp -o /tmp/parcel_uf_check
//   /tmp/parcel_uf_check
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../crop2seg_amd/csrc/parcels_uf.h"

namespace {

struct Case {
    std::string name;
    int B, H, W;
    std::vector<unsigned char> mask;
};

Case make(const std::string& name, int B, int H, int W, const std::function<bool(int, int, int)>& f) {
    Case c{name, B, H, W, std::vector<unsigned char>((size_t)B * H * W)};
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) c.mask[((size_t)b * H + y) * W + x] = f(b, y, x) ? 1 : 0;
    return c;
}

// flood fill, 4-connectivity, inside one image: root[i] = smallest index of the component of i, -1 off the mask
std::vector<int> flood(const Case& c) {
    const int n = c.B * c.H * c.W;
    std::vector<int> root(n, -1), stack;
    for (int s = 0; s < n; ++s) {
        if (!c.mask[s] || root[s] >= 0) continue;
        root[s] = s;
        stack.push_back(s);
        while (!stack.empty()) {
            const int i = stack.back();
            stack.pop_back();
            const int x = i % c.W, y = (i / c.W) % c.H;
            const int nb[4] = {x > 0 ? i - 1 : -1, x < c.W - 1 ? i + 1 : -1, y > 0 ? i - c.W : -1, y < c.H - 1 ? i + c.W : -1};
            for (int j : nb)
                if (j >= 0 && c.mask[j] && root[j] < 0) { root[j] = s; stack.push_back(j); }
        }
    }
    return root;
}

int check(const Case& c, bool reverse) {
    const int n = c.B * c.H * c.W, cap = c.H * c.W;
    std::vector<int> parent(n);
    for (int i = 0; i < n; ++i) parent[i] = i;
    for (int k = 0; k < n; ++k) {
        const int i = reverse ? n - 1 - k : k;
        if (c.mask[i] && !puf_unite_pixel(parent.data(), c.mask.data(), i, c.H, c.W, cap)) {
            std::printf("%s: cap hit while uniting pixel %d\n", c.name.c_str(), i);
            return 1;
        }
    }
    const std::vector<int> want = flood(c);
    for (int i = 0; i < n; ++i) {
        if (!c.mask[i]) continue;
        const int r = puf_find(parent.data(), i, cap);
        if (r != want[i]) {
            std::printf("%s: pixel %d has root %d, flood fill says %d\n", c.name.c_str(), i, r, want[i]);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    const int B = 3, H = 37, W = 53;
    std::vector<Case> cases;
    cases.push_back(make("empty", B, H, W, [](int, int, int) { return false; }));
    cases.push_back(make("full", B, H, W, [](int, int, int) { return true; }));
    cases.push_back(make("serpentine", B, H, W, [&](int, int y, int x) {
        return y % 2 == 0 || (y % 4 == 1 ? x == W - 1 : x == 0);
    }));
    cases.push_back(make("comb", B, H, W, [&](int, int y, int x) { return x % 2 == 0 || y == H - 1; }));
    cases.push_back(make("checkerboard", B, H, W, [](int b, int y, int x) { return (x + y + b) % 2 == 0; }));
    cases.push_back(make("antidiagonal", B, H, W, [&](int, int y, int x) { return x + y == H - 1; }));
    cases.push_back(make("ring", B, H, W, [](int, int y, int x) {
        const bool ring = y >= 5 && y <= 25 && x >= 5 && x <= 40 && (y == 5 || y == 25 || x == 5 || x == 40);
        return ring || (y >= 12 && y <= 15 && x >= 20 && x <= 24);
    }));
    cases.push_back(make("touching", B, H, W, [&](int b, int y, int x) {
        if (b == 0 && y == H - 1 && x >= 10 && x < 20) return true;      // last row of image 0 ...
        if (b == 1 && y == 0 && x >= 10 && x < 20) return true;          // ... first row of image 1, same columns
        if (b == 2 && y == 7 && x >= W - 4) return true;                 // end of a row ...
        if (b == 2 && y == 8 && x < 4) return true;                      // ... start of the next
        return false;
    }));
    unsigned s = 12345u;
    cases.push_back(make("random", 2, 61, 59, [&](int, int, int) {
        s = s * 1664525u + 1013904223u;
        return (s >> 16) % 100 < 60;
    }));
    cases.push_back(make("single", 1, 1, 1, [](int, int, int) { return true; }));
    cases.push_back(make("row", 2, 1, 9, [](int, int, int x) { return x != 4; }));
    cases.push_back(make("column", 2, 9, 1, [](int, int y, int) { return y != 4; }));
    int bad = 0;
    for (const Case& c : cases) {
        bad += check(c, false);
        bad += check(c, true);
    }
    // a damaged parent array ends at the cap instead of spinning
    int cyc[3] = {1, 2, 1};
    if (puf_find(cyc, 0, 3) != -1 || puf_unite(cyc, 0, 2, 3)) { std::printf("cap: a cycle was not reported\n"); ++bad; }
    std::printf(bad ? "FAILED\n" : "parcel_uf_check ok: %zu masks, both orders\n", cases.size());
    return bad ? 1 : 0;
}
