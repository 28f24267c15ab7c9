// bbme_subpel_interpolate_bgr_host (csrc/bbme_host.cpp, the reference of the GPU tests of the BGR SUBPEL INTERPOLATION RULE) under
// AddressSanitizer and UBSan, as a program of its own: the luma planes, the colour frames and the output are exactly sized
// vectors, so a tap read outside a frame or a byte written outside the output is a finding.  The luma planes are flat, so every
// valid moved hypothesis ties at cost 0 and the forward one is selected wherever it is valid: the grids put P1 and P2 on the
// first and last legal quarter-pel position of each axis, one quarter pel and one pixel past them, far outside and on the int16
// extremes, for every phase of a few dens, with odd, even and no paddings.  Checked besides the sanitizers' silence: with
// B = G = R every channel is the grey rule's unpadded window, and zero grids give the in-place blend.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bbme.h"

static const uint8_t FILL8 = 0xA5;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint32_t g_seed = 2025;
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
    // frame width, height, pad_x, pad_y: odd pads, one odd pad, even pads, none
    const int shapes[4][4] = {{14, 10, 1, 1}, {34, 24, 1, 0}, {12, 20, 2, 2}, {16, 12, 0, 0}};
    const int phases[6][2] = {{1, 2}, {1, 3}, {2, 3}, {3, 4}, {254, 255}, {77, 256}};
    for (const auto &sh : shapes) {
        const int w = sh[0], h = sh[1], px = sh[2], py = sh[3], W0 = w + 2 * px, H0 = h + 2 * py, cw = W0 / 2, ch = H0 / 2;
        std::vector<uint8_t> flat((size_t)W0 * H0, 77), l1(flat.size()), l2(flat.size());
        std::vector<uint8_t> c1((size_t)w * h * 3), c2(c1.size()), g1(c1.size()), g2(c1.size());
        for (auto &x : c1) x = (uint8_t)rnd(256);
        for (auto &x : c2) x = (uint8_t)rnd(256);
        for (auto &x : l1) x = 0;
        for (auto &x : l2) x = 0;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const uint8_t a = (uint8_t)rnd(256), b = (uint8_t)(a ^ (uint8_t)rnd(8));
                l1[(size_t)(y + py) * W0 + x + px] = a;
                l2[(size_t)(y + py) * W0 + x + px] = b;
                for (int c = 0; c < 3; ++c) { g1[((size_t)y * w + x) * 3 + c] = a; g2[((size_t)y * w + x) * 3 + c] = b; }
            }
        for (int variant = 0; variant < 7; ++variant) {
            std::vector<int16_t> qf((size_t)cw * ch * 2), qb(qf.size());
            for (int cy = 0; cy < ch; ++cy)
                for (int cx = 0; cx < cw; ++cx) {
                    const size_t c = (size_t)cy * cw + cx;
                    const int k = (int)c + 3 * variant;
                    if (variant < 4) {                     // the far end of the forward vector, and of the reversed backward one
                        qf[2 * c] = sat16(edge_target(k, W0) - 8 * cx);
                        qf[2 * c + 1] = sat16(edge_target(k / 3 + variant, H0) - 8 * cy);
                        qb[2 * c] = sat16(-(edge_target(k + 5, W0) - 8 * cx));
                        qb[2 * c + 1] = sat16(-(edge_target(k / 2 + 1, H0) - 8 * cy));
                    } else if (variant == 4) {             // small vectors: every fraction, most cells valid
                        qf[2 * c] = (int16_t)(rnd(29) - 14); qf[2 * c + 1] = (int16_t)(rnd(29) - 14);
                        qb[2 * c] = (int16_t)(rnd(29) - 14); qb[2 * c + 1] = (int16_t)(rnd(29) - 14);
                    } else if (variant == 5) {             // the int16 extremes
                        const int16_t e[6] = {-32768, 32767, -32767, 0, 3, -1};
                        qf[2 * c] = e[rnd(6)]; qf[2 * c + 1] = e[rnd(6)];
                        qb[2 * c] = e[rnd(6)]; qb[2 * c + 1] = e[rnd(6)];
                    } else {                               // zero grids
                        qf[2 * c] = qf[2 * c + 1] = qb[2 * c] = qb[2 * c + 1] = 0;
                    }
                }
            for (const auto &ph : phases) {
                const int num = ph[0], den = ph[1];
                // flat luma planes: the forward hypothesis is selected wherever it is valid, so the colour taps reach every edge
                std::vector<uint8_t> out((size_t)w * h * 3, FILL8), out2(out.size(), FILL8);
                CHECK(bbme_subpel_interpolate_bgr_host(flat.data(), flat.data(), W0, H0, c1.data(), c2.data(), w, h, px, py, qf.data(),
                                                       qb.data(), num, den, out.data()) == BBME_OK);
                CHECK(bbme_subpel_interpolate_bgr_host(flat.data(), flat.data(), W0, H0, c1.data(), c2.data(), w, h, px, py, qf.data(),
                                                       nullptr, num, den, out2.data()) == BBME_OK);
                if (variant == 6)                          // property 3: the in-place blend
                    for (size_t n = 0; n < out.size(); ++n)
                        CHECK(out[n] == (uint8_t)(((den - num) * c1[n] + num * c2[n] + den / 2) / den) && out2[n] == out[n]);
                // the colour's own lumas (zero border), grey frames: property 1, every channel the grey rule's window
                std::vector<uint8_t> grey((size_t)W0 * H0, FILL8), col((size_t)w * h * 3, FILL8);
                CHECK(bbme_subpel_interpolate_host(l1.data(), l2.data(), W0, H0, qf.data(), qb.data(), num, den, nullptr, grey.data(),
                                                   nullptr, nullptr) == BBME_OK);
                CHECK(bbme_subpel_interpolate_bgr_host(l1.data(), l2.data(), W0, H0, g1.data(), g2.data(), w, h, px, py, qf.data(),
                                                       qb.data(), num, den, col.data()) == BBME_OK);
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x)
                        for (int c = 0; c < 3; ++c)
                            CHECK(col[((size_t)y * w + x) * 3 + c] == grey[(size_t)(y + py) * W0 + x + px]);
            }
            // refusals write nothing
            std::vector<uint8_t> o((size_t)w * h * 3, FILL8);
            CHECK(bbme_subpel_interpolate_bgr_host(flat.data(), flat.data(), W0, H0, c1.data(), c2.data(), w, h, px + 1, py, qf.data(),
                                                   qb.data(), 1, 2, o.data()) == BBME_ERR_INVALID);
            CHECK(bbme_subpel_interpolate_bgr_host(flat.data(), flat.data(), W0, H0, c1.data(), c2.data(), w, h, px, py, qf.data(),
                                                   qb.data(), 2, 2, o.data()) == BBME_ERR_INVALID);
            for (uint8_t x : o) CHECK(x == FILL8);
        }
    }
    printf("subpel interpolation bgr host rule ok\n");
    return 0;
}
