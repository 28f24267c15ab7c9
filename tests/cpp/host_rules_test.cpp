// The CPU rules of csrc/bbme_host.cpp (the references of the GPU tests) under AddressSanitizer and UBSan, as a program of its
// own: every output goes into an exactly sized vector, the grids put vectors on the last legal position, one past it on each side
// and far outside, and every rule that takes a window is called with none, the whole one, a 1x1 window at each corner (and at
// every other position) and the four illegal ones, which must fail with BBME_ERR_INVALID and write nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "bbme.h"

typedef unsigned long long u64;
static const uint8_t FILL8 = 0xA5;
static const int16_t FILL16 = 0x5A5A;
static const u64 FILL64 = 0xDEADBEEFDEADBEEFull;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: %s: CHECK(%s) failed\n", __FILE__, __LINE__, g_what, #cond); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)
static const char *g_what = "";

static uint32_t g_seed = 12345;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

static std::vector<uint8_t> noise(size_t n, int levels)
{
    std::vector<uint8_t> v(n);
    for (auto &x : v) x = (uint8_t)(rnd(levels) * (255 / (levels - 1)));
    return v;
}

// A grid of cols x rows vectors for cells of `cell` pixels whose block of `span` pixels must stay inside w x h: per axis the
// target position cycles through the first and last legal one, one past each, the plane's size, far outside both ways and the
// cell's own position.
static std::vector<int16_t> edge_grid(int cols, int rows, int cell, int span, int w, int h, int phase)
{
    std::vector<int16_t> g((size_t)cols * rows * 2);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const int k = y * cols + x + phase;
            const int tx[9] = {0, -1, w - span, w - span + 1, w, -3000, 3000, x * cell, w - 1};
            const int ty[9] = {0, -1, h - span, h - span + 1, h, -3000, 3000, y * cell, h - 1};
            g[2 * ((size_t)y * cols + x)] = (int16_t)(tx[k % 9] - x * cell);
            g[2 * ((size_t)y * cols + x) + 1] = (int16_t)(ty[(k / 2 + k) % 9] - y * cell);
        }
    return g;
}

struct Outputs {                       // what one call wrote: every buffer exactly as large as the rule says
    std::vector<uint8_t> plane, map;
    std::vector<int16_t> q4;
    std::vector<u64> stats;
    Outputs(size_t plane_n, size_t map_n, size_t q4_n) : plane(plane_n, FILL8), map(map_n, FILL8), q4(q4_n, FILL16), stats(4, FILL64) {}
    bool untouched() const
    {
        for (auto v : plane) if (v != FILL8) return false;
        for (auto v : map) if (v != FILL8) return false;
        for (auto v : q4) if (v != FILL16) return false;
        for (auto v : stats) if (v != FILL64) return false;
        return true;
    }
};

// call(window, outputs) -> status.  The window is over lw x lh units; the statistics of disjoint windows add up.  Returns the
// first statistic over everything.
static u64 windows(const char *what, int lw, int lh, size_t plane_n, size_t map_n, size_t q4_n,
                    const std::function<int(const int *, Outputs &)> &call)
{
    g_what = what;
    Outputs all(plane_n, map_n, q4_n), whole(plane_n, map_n, q4_n);
    CHECK(call(nullptr, all) == BBME_OK);
    const int full[4] = {0, 0, lw, lh};
    CHECK(call(full, whole) == BBME_OK);
    CHECK(all.plane == whole.plane && all.map == whole.map && all.q4 == whole.q4 && all.stats == whole.stats);
    for (auto v : all.stats) CHECK(v != FILL64);
    // 1x1 windows: the four corners first, then every other position; the maps do not depend on the window and the sums add up
    u64 sum[4] = {0, 0, 0, 0};
    const int corners[4][2] = {{0, 0}, {lw - 1, 0}, {0, lh - 1}, {lw - 1, lh - 1}};
    for (int k = 0; k < 4 + lw * lh; ++k) {
        const int x = k < 4 ? corners[k][0] : (k - 4) % lw, y = k < 4 ? corners[k][1] : (k - 4) / lw;
        const int one[4] = {x, y, 1, 1};
        Outputs o(plane_n, map_n, q4_n);
        CHECK(call(one, o) == BBME_OK);
        CHECK(o.plane == all.plane && o.map == all.map && o.q4 == all.q4);
        if (k >= 4)
            for (int i = 0; i < 4; ++i) sum[i] += o.stats[i];
    }
    for (int i = 0; i < 4; ++i) CHECK(sum[i] == all.stats[i]);
    // the four illegal windows: refused, nothing written
    const int bad[4][4] = {{-1, 0, 1, 1}, {0, 0, 0, 1}, {1, 0, lw, 1}, {0, 1, 1, lh}};
    for (const auto &b : bad) {
        Outputs o(plane_n, map_n, q4_n);
        CHECK(call(b, o) == BBME_ERR_INVALID);
        CHECK(bbme_last_error()[0] != 0);
        CHECK(o.untouched());
    }
    return all.stats[0];
}

int main()
{
    const int W = 12, H = 10, CW = W / 2, CH = H / 2;          // planes of 6 x 5 cells
    const int FW = 10, FH = 8, PAD = 1;                        // colour frames: the same padded view
    const size_t NP = (size_t)W * H, NC = (size_t)CW * CH, NF = (size_t)FW * FH * 3;
    const auto p1 = noise(NP, 4), p2 = noise(NP, 4), p3 = noise(NP, 4);
    const auto f1 = noise(NF, 4), f2 = noise(NF, 4), f3 = noise(NF, 4);

    u64 refined = 0;
    for (int phase = 0; phase < 9; ++phase) {
        const auto ga = edge_grid(CW, CH, 2, 2, W, H, phase), gb = edge_grid(CW, CH, 2, 2, W, H, phase + 4);

        for (int tol = 0; tol <= 2; tol += 2)
            windows("consistency", CW, CH, 0, NC, 0, [&](const int *win, Outputs &o) {
                return bbme_cells_consistency_host(ga.data(), gb.data(), CW, CH, tol, win, o.map.data(), o.stats.data());
            });

        const int phases[4][2] = {{1, 2}, {1, 3}, {2, 3}, {255, 256}};
        for (const auto &ph : phases) {
            for (int both = 0; both < 2; ++both)
                windows("interpolation", CW, CH, NP, NC, 0, [&](const int *win, Outputs &o) {
                    return bbme_interpolate_host(p1.data(), p2.data(), W, H, ga.data(), both ? gb.data() : nullptr, ph[0], ph[1], win,
                                                 o.plane.data(), o.map.data(), o.stats.data());
                });
            // the BGR interpolation takes no window: the luma planes of the padded view, the colour frames inside it
            g_what = "interpolation BGR";
            std::vector<uint8_t> out(NF, FILL8);
            CHECK(bbme_interpolate_bgr_host(p1.data(), p2.data(), W, H, f1.data(), f2.data(), FW, FH, PAD, PAD, ga.data(), gb.data(),
                                            ph[0], ph[1], out.data()) == BBME_OK);
            CHECK(bbme_interpolate_bgr_host(p1.data(), p2.data(), W, H, f1.data(), f2.data(), FW, FH, PAD, PAD, ga.data(), nullptr,
                                            ph[0], ph[1], out.data()) == BBME_OK);
            std::vector<uint8_t> keep(NF, FILL8);
            CHECK(bbme_interpolate_bgr_host(p1.data(), p2.data(), W, H, f1.data(), f2.data(), FW, FH, PAD, PAD + 1, ga.data(), gb.data(),
                                            ph[0], ph[1], keep.data()) == BBME_ERR_INVALID);
            for (auto v : keep) CHECK(v == FILL8);
        }

        const int strengths[3] = {1, 200, 1021};
        for (int thr : strengths)
            for (int sides = 1; sides <= 3; ++sides) {              // previous only, next only, both
                const bool hp = sides & 1, hn = sides & 2;
                windows("temporal filter", CW, CH, NP, NC, 0, [&](const int *win, Outputs &o) {
                    return bbme_temporal_filter_host(hp ? p1.data() : nullptr, p2.data(), hn ? p3.data() : nullptr, W, H,
                                                     hp ? ga.data() : nullptr, hn ? gb.data() : nullptr, thr, win, o.plane.data(),
                                                     o.map.data(), o.stats.data());
                });
                windows("temporal filter BGR", CW, CH, NF, NC, 0, [&](const int *win, Outputs &o) {
                    return bbme_temporal_filter_bgr_host(hp ? f1.data() : nullptr, f2.data(), hn ? f3.data() : nullptr, FW, FH, PAD, PAD,
                                                         hp ? ga.data() : nullptr, hn ? gb.data() : nullptr, thr, win, o.plane.data(),
                                                         o.map.data(), o.stats.data());
                });
                // B = G = R without padding is the grey rule: the same map, the first three statistics, three times the fourth
                g_what = "temporal filter, grey against B = G = R";
                std::vector<uint8_t> c1(NP * 3), c2(NP * 3), c3(NP * 3);
                for (size_t i = 0; i < NP * 3; ++i) { c1[i] = p1[i / 3]; c2[i] = p2[i / 3]; c3[i] = p3[i / 3]; }
                Outputs grey(NP, NC, 0), col(NP * 3, NC, 0);
                CHECK(bbme_temporal_filter_host(hp ? p1.data() : nullptr, p2.data(), hn ? p3.data() : nullptr, W, H,
                                                hp ? ga.data() : nullptr, hn ? gb.data() : nullptr, thr, nullptr, grey.plane.data(),
                                                grey.map.data(), grey.stats.data()) == BBME_OK);
                CHECK(bbme_temporal_filter_bgr_host(hp ? c1.data() : nullptr, c2.data(), hn ? c3.data() : nullptr, W, H, 0, 0,
                                                    hp ? ga.data() : nullptr, hn ? gb.data() : nullptr, thr, nullptr, col.plane.data(),
                                                    col.map.data(), col.stats.data()) == BBME_OK);
                CHECK(grey.map == col.map);
                for (size_t i = 0; i < NP * 3; ++i) CHECK(col.plane[i] == grey.plane[i / 3]);
                CHECK(col.stats[0] == grey.stats[0] && col.stats[1] == grey.stats[1] && col.stats[2] == grey.stats[2]);
                CHECK(col.stats[3] == 3 * grey.stats[3]);
            }

        // subpel: I1's 8x8 window at the cell's origin - 3 and I2's 10x10 patch at it + v - 1 must lie inside.  On 12 x 10 no
        // cell's patch does (every cell takes the "not refined" branch); on 16 x 14 the cells (2..5, 2..4) can be refined and
        // the grid puts their patches on the first and last legal position and one past them
        const int sub[2][2] = {{W, H}, {16, 14}};
        for (const auto &wh : sub) {
            const int w = wh[0], h = wh[1], cw = w / 2, ch = h / 2;
            g_seed = 777 + phase;
            const auto i1 = noise((size_t)w * h, 6), i2 = noise((size_t)w * h, 6);
            // the patch's origin b = (2 cx - 3) + v is legal in 2 .. w - 10: edge_grid aims 2 cx + v at 0 .. w - 12, so v + 5
            auto g = edge_grid(cw, ch, 2, 8, w - 4, h - 4, phase);
            for (size_t i = 0; i < g.size(); ++i) g[i] = (int16_t)(g[i] + 5);
            refined += windows("subpel", cw, ch, 0, 0, (size_t)cw * ch * 2, [&](const int *win, Outputs &o) {
                return bbme_subpel_host(i1.data(), i2.data(), w, h, g.data(), win, o.q4.data(), o.stats.data());
            });
        }

        // motion compensation: the window is in pixels of the plane
        const int blocks[3][2] = {{2, 2}, {4, 4}, {4, 2}};            // (grid block, block)
        for (const auto &gbk : blocks) {
            const int cols = (W + gbk[0] - 1) / gbk[0], rows = (H + gbk[0] - 1) / gbk[0];
            const auto g = edge_grid(cols, rows, gbk[0], gbk[1], W, H, phase);
            windows("motion compensation", W, H, NP, 0, 0, [&](const int *win, Outputs &o) {
                return bbme_motion_compensate_host(p1.data(), p2.data(), W, H, g.data(), gbk[0], gbk[1], 7, win, o.plane.data(),
                                                   o.stats.data());
            });
        }
    }
    g_what = "subpel";
    CHECK(refined > 0);                                           // some cells of the 16 x 14 plane took the refining branch
    printf("host rules ok\n");
    return 0;
}
