// The host call of the BGR GLOBAL COMPENSATION RULE (csrc/bbme_host.cpp, the reference of the GPU tests of K18b) under
// AddressSanitizer and UBSan, as a program of its own: the two colour frames and the output are vectors of EXACTLY
// pitch (H - 1) + 3 W bytes (pitch 3 W, and larger ones whose last row ends with its pixels), so a byte read or written outside the
// frames' W x H pixels is a finding, and so is a signed overflow; odd pads; the identity, translations into the padding and out of
// the plane, all sixteen fraction pairs, an edge-straddling affine model and the int32 extremes; windows: none, corners, cutting
// ones, and illegal ones, which must fail and write nothing.  B = G = R frames are checked against the grey rule on the padded plane.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bbme.h"

typedef unsigned long long u64;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint32_t g_seed = 2027;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

struct Model { int32_t m[6]; int unit; };

int main()
{
    const int geoms[4][4] = {{38, 22, 1, 1}, {34, 24, 3, 1}, {40, 30, 0, 0}, {6, 4, 1, 3}};      // W, H, pad_x, pad_y (W0, H0 even)
    std::vector<Model> models = {
        {{0, 0, 0, 0, 0, 0}, 1},
        {{0, 0, 0, 0, 0, 0}, 4},
        {{3 << 16, 0, 0, -(2 << 16), 0, 0}, 1},
        {{-(38 << 16), 0, 0, 22 << 16, 0, 0}, 1},                         // into the padding and beyond
        {{20000, 9000, -2400, -9000, 2400, 9000}, 1},                     // zoom and rotation: sources cross every edge
        {{80000, 36000, -9600, -36000, 9600, 36000}, 4},
        {{INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MIN}, 1},
        {{INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MAX}, 4},
        {{INT32_MAX, 0, 0, 0, 0, INT32_MIN}, 1},
    };
    for (int fx = 0; fx < 4; ++fx)
        for (int fy = 0; fy < 4; ++fy) models.push_back({{(4 + fx) << 16, 0, 0, -((8 - fy) << 16), 0, 0}, 4});
    u64 compensated = 0, skipped_all = 0;
    for (const auto &g : geoms) {
        const int W = g[0], H = g[1], px = g[2], py = g[3], W0 = W + 2 * px, H0 = H + 2 * py;
        for (int extra : {0, 1, 5}) {
            const int pitch = 3 * W + extra, opitch = 3 * W + (extra ? 7 - extra : 0);
            const size_t in_bytes = (size_t)pitch * (H - 1) + (size_t)3 * W, out_bytes = (size_t)opitch * (H - 1) + (size_t)3 * W;
            std::vector<uint8_t> c1(in_bytes), c2(in_bytes);
            for (auto &v : c1) v = (uint8_t)rnd(256);
            for (auto &v : c2) v = (uint8_t)rnd(256);
            const int wins[6][4] = {{0, 0, W, H}, {0, 0, 1, 1}, {W - 1, 0, 1, 1}, {0, H - 1, 1, 1}, {W - 1, H - 1, 1, 1}, {1, 1, W - 2, H - 2}};
            for (size_t mi = 0; mi < models.size(); ++mi) {
                const Model &M = models[mi];
                for (int wi = -1; wi < 6; ++wi) {
                    const int *win = wi < 0 ? nullptr : wins[wi];
                    const u64 area = wi < 0 ? (u64)W * H : (u64)win[2] * win[3];
                    const int fill = (int)((mi * 7 + (size_t)(wi + 1) * 85) % 256);
                    std::vector<uint8_t> out(out_bytes, 0xA5), out2(out_bytes, 0x5A);
                    u64 st[4] = {1, 1, 1, 1}, st2[4] = {2, 2, 2, 2};
                    CHECK(bbme_global_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, M.m, M.unit, fill, win, out.data(),
                                                          opitch, st) == BBME_OK);
                    CHECK(st[2] + st[3] == area);
                    CHECK(st[0] <= st[2] * 3 * 255 * 255 && st[1] <= st[2] * 3 * 255);
                    // the frame alone and the statistics alone give the same; the statistics do not depend on fill
                    CHECK(bbme_global_compensate_bgr_host(nullptr, c2.data(), W, H, pitch, px, py, M.m, M.unit, fill, nullptr, out2.data(),
                                                          opitch, nullptr) == BBME_OK);
                    CHECK(bbme_global_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, M.m, M.unit, 255 - fill, win, nullptr,
                                                          0, st2) == BBME_OK);
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < 3 * W; ++x) CHECK(out[(size_t)y * opitch + x] == out2[(size_t)y * opitch + x]);
                    for (int y = 0; y + 1 < H; ++y)
                        for (int x = 3 * W; x < opitch; ++x) CHECK(out[(size_t)y * opitch + x] == 0xA5);      // between the rows
                    for (int k = 0; k < 4; ++k) CHECK(st[k] == st2[k]);
                    if (mi < 2) {                                         // the identity returns frame 2
                        for (int y = 0; y < H; ++y)
                            for (int x = 0; x < 3 * W; ++x) CHECK(out[(size_t)y * opitch + x] == c2[(size_t)y * pitch + x]);
                        CHECK(st[3] == 0);
                    }
                    if (wi < 0) { compensated += st[2]; skipped_all += st[2] == 0; }
                }
            }
            // B = G = R: every channel is the crop of the grey rule on the zero-padded plane, sse and sad three times its
            std::vector<uint8_t> g1((size_t)W0 * H0, 0), g2((size_t)W0 * H0, 0), k1(in_bytes, 0), k2(in_bytes, 0);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const uint8_t a = (uint8_t)rnd(256), b = (uint8_t)rnd(256);
                    g1[(size_t)(y + py) * W0 + x + px] = a; g2[(size_t)(y + py) * W0 + x + px] = b;
                    for (int c = 0; c < 3; ++c) { k1[(size_t)y * pitch + 3 * x + c] = a; k2[(size_t)y * pitch + 3 * x + c] = b; }
                }
            for (const Model &M : models) {
                std::vector<uint8_t> out(out_bytes, 0), grey((size_t)W0 * H0, 0);
                u64 st[4], gs[4];
                const int win[4] = {px, py, W, H};
                CHECK(bbme_global_compensate_bgr_host(k1.data(), k2.data(), W, H, pitch, px, py, M.m, M.unit, 9, nullptr, out.data(), opitch,
                                                      st) == BBME_OK);
                CHECK(bbme_global_compensate_host(g1.data(), g2.data(), W0, H0, M.m, M.unit, 9, win, grey.data(), gs) == BBME_OK);
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x)
                        for (int c = 0; c < 3; ++c) CHECK(out[(size_t)y * opitch + 3 * x + c] == grey[(size_t)(y + py) * W0 + x + px]);
                CHECK(st[0] == 3 * gs[0] && st[1] == 3 * gs[1] && st[2] == gs[2] && st[3] == gs[3]);
            }
            // refusals write nothing
            std::vector<uint8_t> out(out_bytes, 0xA5);
            u64 st[4] = {7, 7, 7, 7};
            const int bad_wins[3][4] = {{0, 0, W + 1, 1}, {-1, 0, 1, 1}, {0, 0, 1, 0}};
            for (const auto &bw : bad_wins)
                CHECK(bbme_global_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, models[0].m, 1, 0, bw, out.data(), opitch,
                                                      st) == BBME_ERR_INVALID);
            CHECK(bbme_global_compensate_bgr_host(c1.data(), c2.data(), W, H, 3 * W - 1, px, py, models[0].m, 1, 0, nullptr, out.data(),
                                                  opitch, st) == BBME_ERR_INVALID);
            CHECK(bbme_global_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, models[0].m, 1, 0, nullptr, out.data(),
                                                  3 * W - 1, st) == BBME_ERR_INVALID);
            CHECK(bbme_global_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, -1, py, models[0].m, 1, 0, nullptr, out.data(),
                                                  opitch, st) == BBME_ERR_INVALID);
            for (uint8_t v : out) CHECK(v == 0xA5);
            for (u64 v : st) CHECK(v == 7);
        }
    }
    CHECK(compensated > 0 && skipped_all >= 3 * 4 * 3);
    printf("global compensation bgr host rule ok\n");
    return 0;
}
