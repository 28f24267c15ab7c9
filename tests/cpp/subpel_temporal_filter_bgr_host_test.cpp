// bbme_subpel_temporal_filter_bgr_host (csrc/bbme_host.cpp, the reference of the GPU tests of the BGR SUBPEL TEMPORAL FILTER RULE)
// under AddressSanitizer and UBSan, as a program of its own: the frames, the grids and every output are exactly sized vectors, so a
// tap of weight 0 or outside the frame that is read, or a byte written outside an output, is a finding.  The call takes packed
// frames (its integer twin's arguments), so the rows are 3 W bytes apart and every frame row but the first starts where the one
// before ends: a read past a row's end is caught by the values, one past the frame by the sanitizer.  Geometries with odd, even and
// no paddings; the grids put s on the first and last legal quarter-pel position of each axis of the PADDED view, one quarter pel
// and one pixel past them, far outside and on the int16 extremes, for each neighbour set and a few strengths; windows: none, 1x1
// at each corner, and illegal ones, which must fail and write nothing.
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

static uint32_t g_seed = 2026;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

// quarter-pel positions 4 o + q that cycle per axis through both edges of a view of `size` pixels: on the last valid position
// with f = 0 and with f != 0, a quarter pel and a pixel past it, far outside
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

int main()
{
    // width, height, pad_x, pad_y: odd paddings (cells straddle the frame's edge), even ones, none, and a tall narrow frame
    const int geoms[4][4] = {{14, 10, 1, 1}, {36, 22, 1, 2}, {12, 12, 2, 0}, {10, 78, 0, 1}};
    const int thrs[4] = {1, 64, 255, 1021};
    for (const auto &gm : geoms) {
        const int w = gm[0], h = gm[1], px = gm[2], py = gm[3], W0 = w + 2 * px, H0 = h + 2 * py, cw = W0 / 2, ch = H0 / 2;
        // nearly flat frames: every valid neighbour passes at strength 1021, the zero border included (a cost of at most 4 x 103)
        std::vector<uint8_t> cur((size_t)w * h * 3), prev(cur.size()), next(cur.size());
        for (size_t n = 0; n < cur.size(); ++n) {
            cur[n] = (uint8_t)(100 + rnd(4)); prev[n] = (uint8_t)(100 + rnd(4)); next[n] = (uint8_t)(100 + rnd(4));
        }
        for (int variant = 0; variant < 6; ++variant) {
            std::vector<int16_t> qp((size_t)cw * ch * 2), qn(qp.size());
            for (int cy = 0; cy < ch; ++cy)
                for (int cx = 0; cx < cw; ++cx) {
                    const size_t c = (size_t)cy * cw + cx;
                    const int k = (int)c + 3 * variant;
                    if (variant < 4) {                     // one axis on an edge position, the other in place or on one too
                        qp[2 * c] = sat16(edge_target(k, W0) - 8 * cx);
                        qp[2 * c + 1] = variant & 1 ? sat16(edge_target(k / 3 + variant, H0) - 8 * cy) : 0;
                        qn[2 * c] = variant & 2 ? sat16(edge_target(k + 5, W0) - 8 * cx) : 0;
                        qn[2 * c + 1] = sat16(edge_target(k / 2 + 1, H0) - 8 * cy);
                    } else if (variant == 4) {             // small vectors: every fraction, most cells valid
                        qp[2 * c] = (int16_t)(rnd(29) - 14); qp[2 * c + 1] = (int16_t)(rnd(29) - 14);
                        qn[2 * c] = (int16_t)(rnd(29) - 14); qn[2 * c + 1] = (int16_t)(rnd(29) - 14);
                    } else {                               // the int16 extremes
                        const int16_t e[4] = {-32768, 32767, -32767, 32766};
                        qp[2 * c] = e[rnd(4)]; qp[2 * c + 1] = e[rnd(4)];
                        qn[2 * c] = e[rnd(4)]; qn[2 * c + 1] = e[rnd(4)];
                    }
                }
            for (int thr : thrs)
                for (int set = 0; set < 3; ++set) {        // both neighbours, the previous one alone, the next one alone
                    const uint8_t *P = set != 2 ? prev.data() : nullptr, *N = set != 1 ? next.data() : nullptr;
                    const int16_t *QP = P ? qp.data() : nullptr, *QN = N ? qn.data() : nullptr;
                    std::vector<uint8_t> out(cur.size(), FILL8), map((size_t)cw * ch, FILL8);
                    std::vector<u64> st(4, FILL64);
                    CHECK(bbme_subpel_temporal_filter_bgr_host(P, cur.data(), N, w, h, px, py, QP, QN, thr, nullptr, out.data(), map.data(),
                                                               st.data()) == BBME_OK);
                    u64 np = 0, nn = 0, ws = 0;
                    for (int cy = 0; cy < ch; ++cy)
                        for (int cx = 0; cx < cw; ++cx) {
                            const size_t c = (size_t)cy * cw + cx;
                            const int wp = map[c] & 15, wn = map[c] >> 4;
                            CHECK(wp <= 8 && wn <= 8);
                            np += wp > 0; nn += wn > 0; ws += (u64)(wp + wn);
                            const bool vp = P && inside(8 * cx + qp[2 * c], W0) && inside(8 * cy + qp[2 * c + 1], H0);
                            const bool vn = N && inside(8 * cx + qn[2 * c], W0) && inside(8 * cy + qn[2 * c + 1], H0);
                            if (!vp) CHECK(wp == 0);
                            if (!vn) CHECK(wn == 0);
                            if (thr == 1021) CHECK((wp > 0) == vp && (wn > 0) == vn);       // flat frames: cost <= 412
                            if (!wp && !wn)                // the cell's pixels inside the frame are C's
                                for (int i = 0; i < 2; ++i)
                                    for (int j = 0; j < 2; ++j) {
                                        const int x = 2 * cx + j - px, y = 2 * cy + i - py;
                                        if (x < 0 || y < 0 || x >= w || y >= h) continue;
                                        for (int k = 0; k < 3; ++k)
                                            CHECK(out[((size_t)y * w + x) * 3 + k] == cur[((size_t)y * w + x) * 3 + k]);
                                    }
                        }
                    CHECK(st[0] == np && st[1] == nn && st[2] == ws && st[3] <= 3060ull * cw * ch);
                    for (uint8_t x : out) CHECK(x != FILL8);                    // every pixel of the frame is written: 100..103 blended
                    if (variant == 5) CHECK(np == 0 && nn == 0 && out == cur);
                    if (variant == 4 && thr == 1021) CHECK(np + nn > 0);
                    // each output alone gives the same bytes
                    std::vector<uint8_t> out2(cur.size(), FILL8), map2((size_t)cw * ch, FILL8);
                    std::vector<u64> st2(4, FILL64);
                    CHECK(bbme_subpel_temporal_filter_bgr_host(P, cur.data(), N, w, h, px, py, QP, QN, thr, nullptr, out2.data(), nullptr, nullptr) == BBME_OK);
                    CHECK(bbme_subpel_temporal_filter_bgr_host(P, cur.data(), N, w, h, px, py, QP, QN, thr, nullptr, nullptr, map2.data(), nullptr) == BBME_OK);
                    CHECK(bbme_subpel_temporal_filter_bgr_host(P, cur.data(), N, w, h, px, py, QP, QN, thr, nullptr, nullptr, nullptr, st2.data()) == BBME_OK);
                    CHECK(out2 == out && map2 == map && st2 == st);
                    // windows: 1x1 at each corner counts that cell; illegal ones fail and write nothing
                    const int corners[4][2] = {{0, 0}, {cw - 1, 0}, {0, ch - 1}, {cw - 1, ch - 1}};
                    for (const auto &cn : corners) {
                        const int win[4] = {cn[0], cn[1], 1, 1};
                        std::vector<u64> s1(4, FILL64);
                        CHECK(bbme_subpel_temporal_filter_bgr_host(P, cur.data(), N, w, h, px, py, QP, QN, thr, win, nullptr, nullptr, s1.data()) == BBME_OK);
                        const uint8_t m = map[(size_t)cn[1] * cw + cn[0]];
                        CHECK(s1[0] == (u64)((m & 15) > 0) && s1[1] == (u64)((m >> 4) > 0) && s1[2] == (u64)((m & 15) + (m >> 4)) && s1[3] <= 3060);
                    }
                    const int bad[4][4] = {{-1, 0, 1, 1}, {0, 0, cw + 1, 1}, {0, ch, 1, 1}, {0, 0, 1, 0}};
                    for (const auto &win : bad) {
                        std::vector<uint8_t> o(cur.size(), FILL8);
                        std::vector<u64> s1(4, FILL64);
                        CHECK(bbme_subpel_temporal_filter_bgr_host(P, cur.data(), N, w, h, px, py, QP, QN, thr, win, o.data(), nullptr, s1.data()) ==
                              BBME_ERR_INVALID);
                        for (uint8_t x : o) CHECK(x == FILL8);
                        for (u64 x : s1) CHECK(x == FILL64);
                    }
                }
        }
    }
    printf("bgr subpel temporal filter host rule ok\n");
    return 0;
}
