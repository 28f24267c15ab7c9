// The five host calls of the GLOBAL MOTION RULE and the GLOBAL COMPENSATION RULE (csrc/bbme_host.cpp, the references of the GPU
// tests) under AddressSanitizer and UBSan, as a program of its own: grids, masks, planes and every output are exactly sized
// vectors, so a byte read or written outside one is a finding, and so is a signed overflow; the grids hold the int16 extremes and
// the values around both ends of the bins, the models the int32 extremes, the tolerances 0 and 2^40; masks with a pitch of their
// own; windows: none, one cell at each corner, cutting ones, and illegal ones, which must fail and write nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bbme.h"

typedef unsigned long long u64;
static const uint8_t FILL8 = 0xA5;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint32_t g_seed = 2026;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

static int16_t special(int k)
{
    const int t[10] = {-32768, 32767, -1025, -1024, -1023, 1022, 1023, 1024, 0, 1};
    return (int16_t)t[k % 10];
}

static const int32_t kModels[6][6] = {
    {0, 0, 0, 0, 0, 0},
    {3 << 16, 0, 0, -(2 << 16), 0, 0},
    {212992, 655, -328, -98304, 328, 655},
    {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MIN},
    {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MAX},
    {INT32_MAX, 0, 0, 0, 0, INT32_MIN},
};

int main()
{
    const int sizes[3][2] = {{18, 10}, {33, 25}, {6, 40}};                // cells
    const long long tols[3] = {0, 65536, 1LL << 40};
    for (const auto &sz : sizes) {
        const int cw = sz[0], ch = sz[1], w = 2 * cw, h = 2 * ch;
        for (int variant = 0; variant < 3; ++variant) {
            std::vector<int16_t> g((size_t)cw * ch * 2);
            for (size_t n = 0; n < g.size(); ++n)
                g[n] = variant == 0 ? (int16_t)(rnd(9) - 4) : variant == 1 ? (rnd(3) ? (int16_t)(rnd(7) - 3) : special(rnd(10))) : (int16_t)5;
            const int pitch = cw + 3;                                     // the last row ends with the row: exactly sized
            std::vector<uint8_t> excl((size_t)pitch * (ch - 1) + cw);
            for (auto &e : excl) e = rnd(3) ? 0 : (uint8_t)(1 + rnd(255));
            const int wins[7][4] = {{0, 0, cw, ch}, {0, 0, 1, 1}, {cw - 1, 0, 1, 1}, {0, ch - 1, 1, 1}, {cw - 1, ch - 1, 1, 1},
                                    {1, 1, cw - 3, ch - 2}, {3, 0, 2, ch}};
            for (int wi = -1; wi < 7; ++wi) {
                const int *win = wi < 0 ? nullptr : wins[wi];
                const u64 cells = wi < 0 ? (u64)cw * ch : (u64)win[2] * win[3];
                for (int m = 0; m < 2; ++m) {
                    const uint8_t *e = m ? excl.data() : nullptr;
                    std::vector<uint32_t> hist(2 * BBME_GM_BINS, 0xA5A5A5A5u);
                    CHECK(bbme_vector_histogram_host(g.data(), cw, ch, e, pitch, win, hist.data()) == BBME_OK);
                    u64 n[2] = {0, 0};
                    for (int b = 0; b < 2 * BBME_GM_BINS; ++b) n[b / BBME_GM_BINS] += hist[b];
                    CHECK(n[0] == n[1] && n[0] <= cells && (m || n[0] == cells));
                    for (const auto &model : kModels)
                        for (long long tol : tols) {
                            std::vector<uint8_t> map((size_t)cw * ch, FILL8);
                            long long words[16];
                            CHECK(bbme_global_moments_host(g.data(), cw, ch, e, pitch, model, tol, win, map.data(), words) == BBME_OK);
                            CHECK((u64)(words[0] + words[1] + words[2]) == cells && (u64)(words[0] + words[1]) == n[0]);
                            for (uint8_t c : map) CHECK(c <= 2);
                            long long again[16];
                            CHECK(bbme_global_moments_host(g.data(), cw, ch, e, pitch, model, tol, win, nullptr, again) == BBME_OK);
                            for (int k = 0; k < 16; ++k) CHECK(again[k] == words[k]);
                            CHECK(bbme_global_moments_host(g.data(), cw, ch, e, pitch, model, tol, win, map.data(), nullptr) == BBME_OK);
                            for (int kind = 0; kind < 2; ++kind) {
                                int32_t solved[6];
                                CHECK(bbme_global_motion_solve_host(words, kind, solved) == BBME_OK);
                                if (words[0] == 0) for (int k = 0; k < 6; ++k) CHECK(solved[k] == 0);
                            }
                        }
                    for (int kind = 0; kind < 2; ++kind)
                        for (long long tol : tols)
                            for (int it = 0; it <= 8; it += 4) {
                                int32_t model[6];
                                long long words[16];
                                std::vector<uint8_t> map((size_t)cw * ch, FILL8);
                                CHECK(bbme_global_motion_host(g.data(), cw, ch, e, pitch, kind, tol, it, win, model, words, map.data()) == BBME_OK);
                                CHECK((u64)(words[0] + words[1] + words[2]) == cells);
                                int32_t alone[6];
                                CHECK(bbme_global_motion_host(g.data(), cw, ch, e, pitch, kind, tol, it, win, alone, nullptr, nullptr) == BBME_OK);
                                for (int k = 0; k < 6; ++k) CHECK(alone[k] == model[k]);
                                if (variant == 2 && !m) {                 // the uniform grid is found exactly
                                    CHECK(model[0] == 5 * 65536 && model[3] == 5 * 65536 && (u64)words[0] == cells && words[3] == 0);
                                    CHECK(model[1] == 0 && model[2] == 0 && model[4] == 0 && model[5] == 0);
                                }
                            }
                }
            }
            // illegal windows fail and write nothing
            const int bad[4][4] = {{-1, 0, 2, 2}, {0, 0, cw + 1, 1}, {0, 0, 0, 1}, {0, ch - 1, 1, 2}};
            for (const auto &b : bad) {
                std::vector<uint32_t> hist(2 * BBME_GM_BINS, 0xA5A5A5A5u);
                CHECK(bbme_vector_histogram_host(g.data(), cw, ch, nullptr, 0, b, hist.data()) == BBME_ERR_INVALID);
                for (uint32_t v : hist) CHECK(v == 0xA5A5A5A5u);
                std::vector<uint8_t> map((size_t)cw * ch, FILL8);
                CHECK(bbme_global_moments_host(g.data(), cw, ch, nullptr, 0, kModels[1], 0, b, map.data(), nullptr) == BBME_ERR_INVALID);
                for (uint8_t c : map) CHECK(c == FILL8);
            }
            // the compensation: exactly sized planes, every model, both units
            std::vector<uint8_t> i1((size_t)w * h), i2((size_t)w * h);
            for (size_t n = 0; n < i1.size(); ++n) { i1[n] = (uint8_t)rnd(256); i2[n] = (uint8_t)rnd(256); }
            const int pwins[4][4] = {{0, 0, w, h}, {w - 1, h - 1, 1, 1}, {1, 1, w - 3, h - 2}, {3, 0, 2, h}};
            for (const auto &model : kModels)
                for (int unit = 1; unit <= 4; unit += 3)
                    for (int wi = -1; wi < 4; ++wi) {
                        const int *win = wi < 0 ? nullptr : pwins[wi];
                        std::vector<uint8_t> out((size_t)w * h, FILL8);
                        u64 st[4], st2[4];
                        CHECK(bbme_global_compensate_host(i1.data(), i2.data(), w, h, model, unit, 7, win, out.data(), st) == BBME_OK);
                        CHECK(st[2] + st[3] == (wi < 0 ? (u64)w * h : (u64)win[2] * win[3]));
                        CHECK(bbme_global_compensate_host(i1.data(), i2.data(), w, h, model, unit, 200, win, nullptr, st2) == BBME_OK);
                        for (int k = 0; k < 4; ++k) CHECK(st[k] == st2[k]);
                        CHECK(bbme_global_compensate_host(nullptr, i2.data(), w, h, model, unit, 7, nullptr, out.data(), nullptr) == BBME_OK);
                    }
            // the whole-pixel property
            for (int unit = 1; unit <= 4; unit += 3) {
                const int tx = 2, ty = -3;
                const int32_t model[6] = {tx * unit * 65536, 0, 0, ty * unit * 65536, 0, 0};
                std::vector<uint8_t> out((size_t)w * h, FILL8);
                CHECK(bbme_global_compensate_host(nullptr, i2.data(), w, h, model, unit, 9, nullptr, out.data(), nullptr) == BBME_OK);
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) {
                        const bool in = y + ty >= 0 && y + ty < h && x + tx >= 0 && x + tx < w;
                        CHECK(out[(size_t)y * w + x] == (in ? i2[(size_t)(y + ty) * w + x + tx] : 9));
                    }
            }
        }
    }
    printf("global motion host rules ok\n");
    return 0;
}
