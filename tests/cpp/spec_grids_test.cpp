// The table of coarse grids a speculative search may read (csrc/spec_grids.hpp): for every block size B = 2 .. 64 and a set
// of level sizes, every entry's largest index -- the cell of the level's last pixel -- must lie inside the buffer the entry
// names, at the capacities the context allocates: (H / B) (W / B) words for small[], (H / 2) (W / 2) for big[].  The buffers here
// have exactly those sizes and the program is built with AddressSanitizer, so an index past the end is also a fault.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spec_grids.hpp"

using namespace bbme;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_level(int width, int height, int B, bool after_first)
{
    const size_t small_cap = (size_t)(width / B) * (height / B), big_cap = (size_t)(width / 2) * (height / 2);
    std::vector<uint32_t> small0(small_cap, 1u), small1(small_cap, 1u), big0(big_cap, 1u), big1(big_cap, 1u);
    CoarseGrid t[kMaxCoarseGrids];
    const int n = fill_coarse_grids(t, width, B, after_first, small0.data(), small1.data(), (uint32_t)small_cap, big0.data(), big1.data(),
                                    (uint32_t)big_cap);
    int lg = 0;
    while ((1 << lg) < B) ++lg;
    CHECK(n == 2 * lg - 1 + (after_first ? 1 : 0) && n >= 1 && n <= kMaxCoarseGrids, "B %d: %d entries", B, n);
    CHECK(t[after_first ? 1 : 0].grid == small0.data() && t[n - 1].cell_shift == (B > 2 ? 1 : lg), "B %d: first / last entry", B);
    uint64_t sum = 0;
    for (int e = 0; e < kMaxCoarseGrids; ++e) {                  // the entries behind n repeat the last one: the kernel may select any
        const CoarseGrid &g = t[e];
        const bool is_small = g.grid == small0.data() || g.grid == small1.data();
        const size_t cap = is_small ? small_cap : big_cap;
        CHECK(is_small || g.grid == big0.data() || g.grid == big1.data(), "B %d entry %d: unknown buffer", B, e);
        CHECK(g.cell_shift >= 1 && g.cell_shift <= lg && g.cols == width >> g.cell_shift, "B %d entry %d: geometry", B, e);
        if (e > 0 && e < n) CHECK(g.cell_shift <= t[e - 1].cell_shift, "B %d entry %d: cells grow", B, e);
        // search_prediction reads the cell of pixel (ci, cj), ci and cj multiples of B below the level's size: the last one, every
        // row's last and every column's last
        const size_t last = coarse_cell(g, height - B, width - B);
        CHECK(last < cap, "B %d %dx%d entry %d: index %zu of %zu", B, width, height, e, last, cap);
        for (int ci = 0; ci < height; ci += B) {
            CHECK(coarse_cell(g, ci, width - B) < cap, "B %d entry %d row %d", B, e, ci);
            if (coarse_cell(g, ci, width - B) < cap) sum += g.grid[coarse_cell(g, ci, width - B)];
        }
        for (int cj = 0; cj < width; cj += B) {
            CHECK(coarse_cell(g, height - B, cj) < cap, "B %d entry %d column %d", B, e, cj);
            if (coarse_cell(g, height - B, cj) < cap) sum += g.grid[coarse_cell(g, height - B, cj)];
        }
    }
    CHECK(sum == (uint64_t)kMaxCoarseGrids * ((uint64_t)(height / B) + (uint64_t)(width / B)), "B %d: cells read", B);
}

int main()
{
    for (int B = 2; B <= 64; B <<= 1)
        for (int after_first = 0; after_first < 2; ++after_first)
            for (int rows : {1, 2, 3, 7})
                for (int cols : {1, 2, 5, 30})
                    check_level(cols * B, rows * B, B, after_first != 0);
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("spec grids ok\n");
    return 0;
}
