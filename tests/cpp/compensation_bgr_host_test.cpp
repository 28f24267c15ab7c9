// The host call of the BGR COMPENSATION RULE (csrc/bbme_host.cpp, the reference of the GPU tests of K11b) under AddressSanitizer
// and UBSan, as a program of its own: the two colour frames, the grid and the output are vectors of EXACTLY
// pitch (rows - 1) + one row of payload (pitch the packed one, and larger ones whose last row ends with its payload), so a byte
// read or written outside the frames' W x H pixels or outside the grid's CH x CW cells is a finding, and so is a signed overflow;
// odd pads, where cells straddle the frame's edge; grids: zero, every fraction pair, cells whose source meets every edge of the
// padded plane, and the int16 extremes (4 G overflows int16 with unit 1), each in both units; windows: none, corners, cutting
// ones, and illegal ones, which must fail and write nothing.  B = G = R frames are checked against the grey rules on the padded
// plane: the subpel compensation rule (unit 4) and the integer compensation rule at block 2 (unit 1).
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

static uint32_t g_seed = 2031;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

// a grid of ch x cw cells, rows gpitch cells apart, in a vector of exactly gpitch (ch - 1) + cw cells
struct Grid {
    std::vector<int16_t> v;
    int cw, ch, pitch;
    Grid(int cw_, int ch_, int pitch_) : v(2 * ((size_t)pitch_ * (ch_ - 1) + cw_), 0x7a7a), cw(cw_), ch(ch_), pitch(pitch_) {}
    int16_t *at(int cx, int cy) { return &v[2 * ((size_t)cy * pitch + cx)]; }
    void set(int cx, int cy, int x, int y) { at(cx, cy)[0] = (int16_t)x; at(cx, cy)[1] = (int16_t)y; }
};

int main()
{
    const int geoms[4][4] = {{38, 22, 1, 1}, {34, 24, 3, 1}, {40, 30, 0, 0}, {6, 4, 1, 3}};      // W, H, pad_x, pad_y (W0, H0 even)
    u64 compensated = 0, skipped = 0;
    for (const auto &g : geoms) {
        const int W = g[0], H = g[1], px = g[2], py = g[3], W0 = W + 2 * px, H0 = H + 2 * py, CW = W0 / 2, CH = H0 / 2;
        for (int extra : {0, 1, 5}) {
            const int pitch = 3 * W + extra, opitch = 3 * W + (extra ? 7 - extra : 0), gpitch = CW + extra;
            const size_t in_bytes = (size_t)pitch * (H - 1) + (size_t)3 * W, out_bytes = (size_t)opitch * (H - 1) + (size_t)3 * W;
            std::vector<uint8_t> c1(in_bytes), c2(in_bytes);
            for (auto &v : c1) v = (uint8_t)rnd(256);
            for (auto &v : c2) v = (uint8_t)rnd(256);
            // the grids: 0 zero, 1 fractions, 2 edges, 3 extremes
            std::vector<Grid> grids(4, Grid(CW, CH, gpitch));
            const int ext[7] = {-32768, 32767, -32765, 32764, 0, 3, -1};
            for (int cy = 0; cy < CH; ++cy)
                for (int cx = 0; cx < CW; ++cx) {
                    const int k = (cy * CW + cx) % 16;
                    grids[0].set(cx, cy, 0, 0);
                    grids[1].set(cx, cy, 4 * (rnd(7) - 3) + (k & 3), 4 * (rnd(7) - 3) + (k >> 2));
                    // the source's first column at -1, 0, W0 - 3, W0 - 2 or W0 - 1 of the padded plane, with every fraction; rows alike
                    const int tx[5] = {-1, 0, W0 - 3, W0 - 2, W0 - 1}, ty[5] = {-1, 0, H0 - 3, H0 - 2, H0 - 1};
                    if ((cx + cy) & 1) grids[2].set(cx, cy, 4 * (tx[rnd(5)] - 2 * cx) + rnd(4), rnd(4));
                    else grids[2].set(cx, cy, rnd(4), 4 * (ty[rnd(5)] - 2 * cy) + rnd(4));
                    if (rnd(10) < 3) grids[3].set(cx, cy, ext[rnd(7)], ext[rnd(7)]);
                    else grids[3].set(cx, cy, rnd(27) - 13, rnd(27) - 13);
                }
            grids[3].set(0, 0, -32768, 32767);
            grids[3].set(CW - 1, CH - 1, 32767, -32768);
            const int wins[6][4] = {{0, 0, W, H}, {0, 0, 1, 1}, {W - 1, 0, 1, 1}, {0, H - 1, 1, 1}, {W - 1, H - 1, 1, 1}, {1, 1, W - 2, H - 2}};
            for (size_t gi = 0; gi < grids.size(); ++gi)
                for (int unit : {1, 4})
                    for (int wi = -1; wi < 6; ++wi) {
                        const int16_t *G = grids[gi].v.data();
                        const int *win = wi < 0 ? nullptr : wins[wi];
                        const u64 area = wi < 0 ? (u64)W * H : (u64)win[2] * win[3];
                        const int fill = (int)((gi * 7 + (size_t)(wi + 1) * 85 + unit) % 256);
                        std::vector<uint8_t> out(out_bytes, 0xA5), out2(out_bytes, 0x5A);
                        u64 st[4] = {1, 1, 1, 1}, st2[4] = {2, 2, 2, 2};
                        CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, G, gpitch, unit, fill, win, out.data(),
                                                       opitch, st) == BBME_OK);
                        CHECK(st[2] + st[3] == area);
                        CHECK(st[0] <= st[2] * 3 * 255 * 255 && st[1] <= st[2] * 3 * 255);
                        // the frame alone and the statistics alone give the same; the statistics do not depend on fill
                        CHECK(bbme_compensate_bgr_host(nullptr, c2.data(), W, H, pitch, px, py, G, gpitch, unit, fill, nullptr, out2.data(),
                                                       opitch, nullptr) == BBME_OK);
                        CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, G, gpitch, unit, 255 - fill, win, nullptr, 0,
                                                       st2) == BBME_OK);
                        for (int y = 0; y < H; ++y)
                            for (int x = 0; x < 3 * W; ++x) CHECK(out[(size_t)y * opitch + x] == out2[(size_t)y * opitch + x]);
                        for (int y = 0; y + 1 < H; ++y)
                            for (int x = 3 * W; x < opitch; ++x) CHECK(out[(size_t)y * opitch + x] == 0xA5);      // between the rows
                        for (int k = 0; k < 4; ++k) CHECK(st[k] == st2[k]);
                        if (gi == 0) {                                    // a zero grid returns frame 2
                            for (int y = 0; y < H; ++y)
                                for (int x = 0; x < 3 * W; ++x) CHECK(out[(size_t)y * opitch + x] == c2[(size_t)y * pitch + x]);
                            CHECK(st[3] == 0);
                        }
                        if (wi < 0) { compensated += st[2]; skipped += st[3]; }
                    }
            // B = G = R: every channel is the crop of the grey rules on the zero-padded plane, sse and sad three times theirs
            std::vector<uint8_t> g1((size_t)W0 * H0, 0), g2((size_t)W0 * H0, 0), k1(in_bytes, 0), k2(in_bytes, 0);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const uint8_t a = (uint8_t)rnd(256), b = (uint8_t)rnd(256);
                    g1[(size_t)(y + py) * W0 + x + px] = a; g2[(size_t)(y + py) * W0 + x + px] = b;
                    for (int c = 0; c < 3; ++c) { k1[(size_t)y * pitch + 3 * x + c] = a; k2[(size_t)y * pitch + 3 * x + c] = b; }
                }
            for (Grid &S : grids) {
                std::vector<int16_t> packed((size_t)2 * CW * CH);         // the grey rules take packed grids
                for (int cy = 0; cy < CH; ++cy)
                    for (int cx = 0; cx < CW; ++cx)
                        for (int k = 0; k < 2; ++k) packed[2 * ((size_t)cy * CW + cx) + k] = S.at(cx, cy)[k];
                for (int unit : {1, 4}) {
                    std::vector<uint8_t> out(out_bytes, 0), grey((size_t)W0 * H0, 0);
                    u64 st[4], gs[4];
                    const int win[4] = {px, py, W, H};
                    CHECK(bbme_compensate_bgr_host(k1.data(), k2.data(), W, H, pitch, px, py, S.v.data(), gpitch, unit, 9, nullptr,
                                                   out.data(), opitch, st) == BBME_OK);
                    if (unit == 4)
                        CHECK(bbme_subpel_compensate_host(g1.data(), g2.data(), W0, H0, packed.data(), 9, win, grey.data(), gs) == BBME_OK);
                    else
                        CHECK(bbme_motion_compensate_host(g1.data(), g2.data(), W0, H0, packed.data(), 2, 2, 9, win, grey.data(), gs) ==
                              BBME_OK);
                    for (int y = 0; y < H; ++y)
                        for (int x = 0; x < W; ++x)
                            for (int c = 0; c < 3; ++c) CHECK(out[(size_t)y * opitch + 3 * x + c] == grey[(size_t)(y + py) * W0 + x + px]);
                    CHECK(st[0] == 3 * gs[0] && st[1] == 3 * gs[1] && st[2] == gs[2] && st[3] == gs[3]);
                }
            }
            // refusals write nothing
            std::vector<uint8_t> out(out_bytes, 0xA5);
            u64 st[4] = {7, 7, 7, 7};
            const int16_t *G = grids[1].v.data();
            const int bad_wins[3][4] = {{0, 0, W + 1, 1}, {-1, 0, 1, 1}, {0, 0, 1, 0}};
            for (const auto &bw : bad_wins)
                CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, G, gpitch, 4, 0, bw, out.data(), opitch, st) ==
                      BBME_ERR_INVALID);
            CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, 3 * W - 1, px, py, G, gpitch, 4, 0, nullptr, out.data(), opitch, st) ==
                  BBME_ERR_INVALID);
            CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, G, gpitch, 4, 0, nullptr, out.data(), 3 * W - 1, st) ==
                  BBME_ERR_INVALID);
            CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, G, CW - 1, 4, 0, nullptr, out.data(), opitch, st) ==
                  BBME_ERR_INVALID);
            CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, px, py, G, gpitch, 2, 0, nullptr, out.data(), opitch, st) ==
                  BBME_ERR_INVALID);
            CHECK(bbme_compensate_bgr_host(c1.data(), c2.data(), W, H, pitch, -1, py, G, gpitch, 4, 0, nullptr, out.data(), opitch, st) ==
                  BBME_ERR_INVALID);
            for (uint8_t v : out) CHECK(v == 0xA5);
            for (u64 v : st) CHECK(v == 7);
        }
    }
    CHECK(compensated > 0 && skipped > 0);
    printf("compensation bgr host rule ok\n");
    return 0;
}
