// bbme_wide_temporal_filter_bgr_host (csrc/bbme_host.cpp, the reference of the GPU tests of the BGR WIDE TEMPORAL FILTER RULE) under
// AddressSanitizer and UBSan, as a program of its own: frames, grids and every output are exactly sized vectors, so a tap of weight
// 0 or of the zero border read outside a frame, a grid word read past a row or a value written outside an output is a finding.
// Paddings odd, even, mixed and none; s on and past every edge of the padded view by a quarter pel (f = 0) and a pixel (f != 0),
// far outside and on the int16 extremes; each of the 15 neighbour sets; windows: none, 1x1 at each corner, and illegal ones, which
// must fail and write nothing.  The frames are nearly flat and so is the zero border's cost (at most 4 x 103 < 1021): at the
// largest strength a weight of 0 is an invalid cell and nothing else.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bbme.h"

typedef unsigned long long u64;
static const uint8_t FILL8 = 0xA5;
static const uint16_t FILL16 = 0xA5A5;
static const u64 FILL64 = 0xDEADBEEFDEADBEEFull;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static uint32_t g_seed = 2027;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

static int edge_target(int k, int size)
{
    const int t[16] = {0, -1, -4, 1, 3, -3, 4 * (size - 2), 4 * (size - 2) + 1, 4 * (size - 3) + 3, 4 * (size - 3) + 1, 4 * (size - 2) + 3,
                       4 * (size - 1), 4 * size, -40000, 40000, 4 * (size - 2) - 1};
    return t[k % 16];
}

static int16_t sat16(int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

// every tap of non-zero weight of a cell at quarter-pel position p (one axis) lies in a view of `size`
static bool inside(int p, int size)
{
    const int i = p >> 2;
    return i >= 0 && i + 2 + ((p & 3) != 0) <= size;
}

static void test_wide_filter_bgr()
{
    // (W, H, pad_x, pad_y): both paddings odd, one odd, both even, none; a last run of 2 cells and whole runs
    const int shapes[5][4] = {{14, 10, 1, 1}, {14, 12, 1, 0}, {34, 22, 2, 2}, {12, 80, 0, 0}, {12, 10, 3, 5}};
    const int thrs[3] = {1, 64, 1021};
    for (const auto &sh : shapes) {
        const int w = sh[0], h = sh[1], px = sh[2], py = sh[3], W0 = w + 2 * px, H0 = h + 2 * py, cw = W0 / 2, ch = H0 / 2;
        std::vector<uint8_t> cur((size_t)3 * w * h), nb[4];
        for (auto &x : cur) x = (uint8_t)(100 + rnd(4));
        for (auto &p : nb) { p.resize((size_t)3 * w * h); for (auto &x : p) x = (uint8_t)(100 + rnd(4)); }
        for (int variant = 0; variant < 4; ++variant) {
            const int pitch = cw + (variant & 1) * 3;
            std::vector<int16_t> q[4];
            for (int k = 0; k < 4; ++k) {
                q[k].assign(2 * ((size_t)pitch * (ch - 1) + cw), 0);
                for (int cy = 0; cy < ch; ++cy)
                    for (int cx = 0; cx < cw; ++cx) {
                        int16_t *v = &q[k][2 * ((size_t)cy * pitch + cx)];
                        const int c = cy * cw + cx + 3 * variant + 5 * k;
                        if (variant < 2) {                     // one axis on an edge position of the padded view, the other in place or on one too
                            v[0] = sat16(edge_target(c, W0) - 8 * cx);
                            v[1] = (variant + k) & 1 ? sat16(edge_target(c / 3 + k, H0) - 8 * cy) : 0;
                        } else if (variant == 2) {             // small vectors: every fraction, most cells valid
                            v[0] = (int16_t)(rnd(29) - 14); v[1] = (int16_t)(rnd(29) - 14);
                        } else {                               // the int16 extremes
                            const int16_t e[4] = {-32768, 32767, -32767, 32766};
                            v[0] = e[rnd(4)]; v[1] = e[rnd(4)];
                        }
                    }
            }
            for (int thr : thrs)
                for (int set = 1; set < 16; ++set) {
                    const uint8_t *frames[4];
                    const int16_t *grids[4];
                    for (int k = 0; k < 4; ++k) {
                        frames[k] = set >> k & 1 ? nb[k].data() : nullptr;
                        grids[k] = set >> k & 1 ? q[k].data() : nullptr;
                    }
                    std::vector<uint8_t> out((size_t)3 * w * h, FILL8);
                    std::vector<uint16_t> map((size_t)cw * ch, FILL16);
                    std::vector<u64> st(6, FILL64);
                    CHECK(bbme_wide_temporal_filter_bgr_host(frames, cur.data(), w, h, px, py, grids, pitch, thr, nullptr, out.data(),
                                                             map.data(), st.data()) == BBME_OK);
                    u64 n[4] = {0, 0, 0, 0}, ws = 0;
                    for (int cy = 0; cy < ch; ++cy)
                        for (int cx = 0; cx < cw; ++cx) {
                            const uint16_t m = map[(size_t)cy * cw + cx];
                            int sum = 0;
                            for (int k = 0; k < 4; ++k) {
                                const int wk = m >> (4 * k) & 15;
                                CHECK(wk <= 8);
                                const int16_t *v = &q[k][2 * ((size_t)cy * pitch + cx)];
                                const bool valid = frames[k] && inside(8 * cx + v[0], W0) && inside(8 * cy + v[1], H0);
                                if (!valid) CHECK(wk == 0);
                                if (thr == 1021) CHECK((wk > 0) == valid);             // flat frames and border: cost <= 412
                                n[k] += wk > 0; sum += wk;
                            }
                            ws += (u64)sum;
                            if (!sum)                          // the cell's pixels inside the frame are C's
                                for (int i = 0; i < 2; ++i)
                                    for (int j = 0; j < 2; ++j) {
                                        const int x = 2 * cx + j - px, y = 2 * cy + i - py;
                                        if (x < 0 || y < 0 || x >= w || y >= h) continue;
                                        for (int c = 0; c < 3; ++c) CHECK(out[((size_t)y * w + x) * 3 + c] == cur[((size_t)y * w + x) * 3 + c]);
                                    }
                        }
                    for (uint8_t x : out) CHECK(x != FILL8);   // every pixel of the frame is written (the frames hold 100 .. 103)
                    CHECK(st[0] == n[0] && st[1] == n[1] && st[2] == n[2] && st[3] == n[3] && st[4] == ws && st[5] <= 3060ull * cw * ch);
                    if (variant == 3) CHECK(ws == 0 && out == cur);
                    if (variant == 2 && thr >= 64) CHECK(ws > 0);
                    // each output alone gives the same bytes
                    std::vector<uint8_t> out2((size_t)3 * w * h, FILL8);
                    std::vector<uint16_t> map2((size_t)cw * ch, FILL16);
                    std::vector<u64> st2(6, FILL64);
                    CHECK(bbme_wide_temporal_filter_bgr_host(frames, cur.data(), w, h, px, py, grids, pitch, thr, nullptr, out2.data(), nullptr,
                                                             nullptr) == BBME_OK);
                    CHECK(bbme_wide_temporal_filter_bgr_host(frames, cur.data(), w, h, px, py, grids, pitch, thr, nullptr, nullptr, map2.data(),
                                                             nullptr) == BBME_OK);
                    CHECK(bbme_wide_temporal_filter_bgr_host(frames, cur.data(), w, h, px, py, grids, pitch, thr, nullptr, nullptr, nullptr,
                                                             st2.data()) == BBME_OK);
                    CHECK(out2 == out && map2 == map && st2 == st);
                    if (set % 5) continue;                     // windows on a third of the sets
                    const int corners[4][2] = {{0, 0}, {cw - 1, 0}, {0, ch - 1}, {cw - 1, ch - 1}};
                    for (const auto &cn : corners) {
                        const int win[4] = {cn[0], cn[1], 1, 1};
                        std::vector<u64> s1(6, FILL64);
                        CHECK(bbme_wide_temporal_filter_bgr_host(frames, cur.data(), w, h, px, py, grids, pitch, thr, win, nullptr, nullptr,
                                                                 s1.data()) == BBME_OK);
                        const uint16_t m = map[(size_t)cn[1] * cw + cn[0]];
                        u64 sum = 0;
                        for (int k = 0; k < 4; ++k) { CHECK(s1[k] == (u64)((m >> (4 * k) & 15) > 0)); sum += m >> (4 * k) & 15; }
                        CHECK(s1[4] == sum && s1[5] <= 3060);
                    }
                    const int bad[4][4] = {{-1, 0, 1, 1}, {0, 0, cw + 1, 1}, {0, ch, 1, 1}, {0, 0, 1, 0}};
                    for (const auto &win : bad) {
                        std::vector<uint8_t> o((size_t)3 * w * h, FILL8);
                        std::vector<u64> s1(6, FILL64);
                        CHECK(bbme_wide_temporal_filter_bgr_host(frames, cur.data(), w, h, px, py, grids, pitch, thr, win, o.data(), nullptr,
                                                                 s1.data()) == BBME_ERR_INVALID);
                        for (uint8_t x : o) CHECK(x == FILL8);
                        for (u64 x : s1) CHECK(x == FILL64);
                    }
                }
        }
    }
}

int main()
{
    test_wide_filter_bgr();
    printf("bgr wide temporal filter host rule ok\n");
    return 0;
}
