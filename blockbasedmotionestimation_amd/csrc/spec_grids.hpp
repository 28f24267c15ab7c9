// spec_grids.hpp -- the coarse grids a speculative search may predict from (FastSearchArgs::late, bbme_kernels.hpp).
// Plain C++: the host fills the table (enqueue order of bbme_device.hip), the search kernel indexes it, and
// tests/cpp/spec_grids_test.cpp checks every entry's largest index against its buffer without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BBME_HD __host__ __device__
#else
#define BBME_HD
#endif

namespace bbme {

// One grid of the coarser level as a sweep leaves it: cells of 1 << cell_shift pixels, `cols` of them per row, pair p of a
// batch `stride` words after pair 0.
struct CoarseGrid {
    const uint32_t *grid;
    uint32_t stride;
    int cell_shift;
    int cols;
};

// 2 log2(B) - 1 grids for a level of B x B blocks: the one its two sweeps at B leave, then two per halving down to 2 x 2; one
// more when the search is forked behind the FIRST sweep at B
constexpr int kMaxCoarseGrids = 12;             // B = 64

// The cell of `g` that covers pixel (ci, cj) of the coarser level (row, column).
BBME_HD inline size_t coarse_cell(const CoarseGrid &g, int ci, int cj)
{
    return (size_t)(ci >> g.cell_shift) * (size_t)g.cols + (size_t)(cj >> g.cell_shift);
}

// The table for a coarser level of `width` pixels per row and `block`-sized blocks (a power of two, 2 .. 64; width a multiple
// of it), in the order its sweeps run.  The sweeps at `block` go small0 -> small1 -> small0 (capacity (H / B) (W / B) words per
// pair each): entry 0 is small0, what the second of them leaves -- or, `after_first`, small1 followed by small0.  Then, per
// halving, the first sweep's grid in big0 and the second's in big1 (capacity (H / 2) (W / 2) each): a sweep at cell size 2^s
// writes (H >> s) (W >> s) <= (H / 2) (W / 2) words, so every entry indexes inside its buffer whichever sweep wrote the
// buffer last.  Returns the number of entries; the rest of the table repeats the last one.
inline int fill_coarse_grids(CoarseGrid (&t)[kMaxCoarseGrids], int width, int block, bool after_first, const uint32_t *small0,
                             const uint32_t *small1, uint32_t small_stride, const uint32_t *big0, const uint32_t *big1,
                             uint32_t big_stride)
{
    int lg = 0;
    while ((1 << lg) < block) ++lg;
    int n = 0;
    if (after_first) t[n++] = CoarseGrid{small1, small_stride, lg, width >> lg};
    t[n++] = CoarseGrid{small0, small_stride, lg, width >> lg};
    for (int s = lg - 1; s >= 1 && n + 2 <= kMaxCoarseGrids; --s) {
        t[n++] = CoarseGrid{big0, big_stride, s, width >> s};
        t[n++] = CoarseGrid{big1, big_stride, s, width >> s};
    }
    for (int i = n; i < kMaxCoarseGrids; ++i) t[i] = t[n - 1];
    return n;
}

}  // namespace bbme
