// bbme_subpel_interpolate_host (csrc/bbme_host.cpp, the reference of the GPU tests of the SUBPEL INTERPOLATION RULE) under
// AddressSanitizer and UBSan, as a program of its own: the planes and every output are exactly sized vectors, so a tap read
// outside the plane or a byte written outside an output is a finding; the grids put P1 and P2 on the first and last legal
// quarter-pel position of each axis, one quarter pel and one pixel past them, far outside and on the int16 extremes, for every
// phase of a few dens; windows: none, the whole grid, 1x1 at each corner, and illegal ones, which must fail and write nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bbme.h"

typedef unsigned long long u64;
static const uint8_t FILL8 = 0xA5;
static const u64 FILL64 = 0xDEADBEEFDEADBEEFull;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint32_t g_seed = 2024;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

// quarter-pel vectors whose far end, 4 o + v, cycles per axis through positions around both edges of a plane of `size` pixels
static int edge_target(int k, int size)
{
    const int t[14] = {0, -1, -4, 1, 4 * (size - 2), 4 * (size - 2) + 1, 4 * (size - 3) + 3, 4 * (size - 3), 4 * (size - 1), 4 * size,
                       -40000, 40000, 4 * (size - 2) - 1, 3};
    return t[k % 14];
}

static int16_t sat16(int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

int main()
{
    const int sizes[3][2] = {{16, 12}, {38, 26}, {12, 80}};
    const int phases[7][2] = {{1, 2}, {1, 3}, {2, 3}, {3, 4}, {2, 5}, {254, 255}, {77, 256}};
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1], cw = w / 2, ch = h / 2;
        std::vector<uint8_t> i1((size_t)w * h), i2((size_t)w * h);
        for (auto &x : i1) x = (uint8_t)rnd(256);
        for (size_t n = 0; n < i2.size(); ++n) i2[n] = (uint8_t)(i1[n] ^ (uint8_t)rnd(16));
        for (int variant = 0; variant < 6; ++variant) {
            std::vector<int16_t> qf((size_t)cw * ch * 2), qb(qf.size());
            for (int cy = 0; cy < ch; ++cy)
                for (int cx = 0; cx < cw; ++cx) {
                    const size_t c = (size_t)cy * cw + cx;
                    const int k = (int)c + 3 * variant;
                    if (variant < 4) {                     // the far end of the forward vector, and of the reversed backward one
                        qf[2 * c] = sat16(edge_target(k, w) - 8 * cx);
                        qf[2 * c + 1] = sat16(edge_target(k / 3 + variant, h) - 8 * cy);
                        qb[2 * c] = sat16(-(edge_target(k + 5, w) - 8 * cx));
                        qb[2 * c + 1] = sat16(-(edge_target(k / 2 + 1, h) - 8 * cy));
                    } else if (variant == 4) {             // small vectors: every fraction, most cells valid
                        qf[2 * c] = (int16_t)(rnd(29) - 14); qf[2 * c + 1] = (int16_t)(rnd(29) - 14);
                        qb[2 * c] = (int16_t)(rnd(29) - 14); qb[2 * c + 1] = (int16_t)(rnd(29) - 14);
                    } else {                               // the int16 extremes
                        const int16_t e[6] = {-32768, 32767, -32767, 0, 3, -1};
                        qf[2 * c] = e[rnd(6)]; qf[2 * c + 1] = e[rnd(6)];
                        qb[2 * c] = e[rnd(6)]; qb[2 * c + 1] = e[rnd(6)];
                    }
                }
            for (const auto &ph : phases) {
                std::vector<uint8_t> out((size_t)w * h, FILL8), sel((size_t)cw * ch, FILL8);
                std::vector<u64> st(4, FILL64);
                CHECK(bbme_subpel_interpolate_host(i1.data(), i2.data(), w, h, qf.data(), qb.data(), ph[0], ph[1], nullptr, out.data(),
                                                   sel.data(), st.data()) == BBME_OK);
                u64 counted[3] = {0, 0, 0};
                for (uint8_t k : sel) { CHECK(k <= 2); ++counted[k]; }
                CHECK(st[0] == counted[0] && st[1] == counted[1] && st[2] == counted[2] && st[0] + st[1] + st[2] == (u64)cw * ch);
                CHECK(st[3] <= 1020ull * cw * ch);
                if (variant == 5) CHECK(counted[2] > 0);
                // without the backward grid nothing selects it; each output alone gives the same bytes
                std::vector<uint8_t> out2((size_t)w * h, FILL8), sel2((size_t)cw * ch, FILL8);
                CHECK(bbme_subpel_interpolate_host(i1.data(), i2.data(), w, h, qf.data(), nullptr, ph[0], ph[1], nullptr, nullptr,
                                                   sel2.data(), nullptr) == BBME_OK);
                for (uint8_t k : sel2) CHECK(k == 0 || k == 2);
                CHECK(bbme_subpel_interpolate_host(i1.data(), i2.data(), w, h, qf.data(), qb.data(), ph[0], ph[1], nullptr, out2.data(),
                                                   nullptr, nullptr) == BBME_OK);
                CHECK(out2 == out);
                // windows: 1x1 at each corner adds up per cell; illegal ones fail and write nothing
                const int corners[4][2] = {{0, 0}, {cw - 1, 0}, {0, ch - 1}, {cw - 1, ch - 1}};
                for (const auto &cn : corners) {
                    const int win[4] = {cn[0], cn[1], 1, 1};
                    std::vector<u64> s1(4, FILL64);
                    CHECK(bbme_subpel_interpolate_host(i1.data(), i2.data(), w, h, qf.data(), qb.data(), ph[0], ph[1], win, nullptr, nullptr,
                                                       s1.data()) == BBME_OK);
                    CHECK(s1[0] + s1[1] + s1[2] == 1 && s1[sel[(size_t)cn[1] * cw + cn[0]]] == 1 && s1[3] <= 1020);
                }
                const int bad[4][4] = {{-1, 0, 1, 1}, {0, 0, cw + 1, 1}, {0, ch, 1, 1}, {0, 0, 1, 0}};
                for (const auto &win : bad) {
                    std::vector<uint8_t> o((size_t)w * h, FILL8);
                    std::vector<u64> s1(4, FILL64);
                    CHECK(bbme_subpel_interpolate_host(i1.data(), i2.data(), w, h, qf.data(), qb.data(), ph[0], ph[1], win, o.data(), nullptr,
                                                       s1.data()) == BBME_ERR_INVALID);
                    for (uint8_t x : o) CHECK(x == FILL8);
                    for (u64 x : s1) CHECK(x == FILL64);
                }
            }
        }
    }
    printf("subpel interpolation host rule ok\n");
    return 0;
}
