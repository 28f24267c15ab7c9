// bbme_subpel_temporal_filter_host (csrc/bbme_host.cpp, the reference of the GPU tests of the SUBPEL TEMPORAL FILTER RULE) under
// AddressSanitizer and UBSan, as a program of its own: the planes and every output are exactly sized vectors, so a tap of weight 0
// read outside the plane or a byte written outside an output is a finding; the grids put s on the first and last legal
// quarter-pel position of each axis, one quarter pel and one pixel past them, far outside and on the int16 extremes, for each
// neighbour set and a few strengths; windows: none, 1x1 at each corner, and illegal ones, which must fail and write nothing.
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

static uint32_t g_seed = 2025;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

// quarter-pel positions 4 o + q that cycle per axis through both edges of a plane of `size` pixels: on the last valid position
// with f = 0 and with f != 0, a quarter pel and a pixel past it, far outside
static int edge_target(int k, int size)
{
    const int t[16] = {0, -1, -4, 1, 3, -3, 4 * (size - 2), 4 * (size - 2) + 1, 4 * (size - 3) + 3, 4 * (size - 3) + 1, 4 * (size - 2) + 3,
                       4 * (size - 1), 4 * size, -40000, 40000, 4 * (size - 2) - 1};
    return t[k % 16];
}

static int16_t sat16(int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

// every tap of non-zero weight of a cell at quarter-pel position p (one axis) lies in a plane of `size`
static bool inside(int p, int size)
{
    const int i = p >> 2;
    return i >= 0 && i + 2 + ((p & 3) != 0) <= size;
}

int main()
{
    const int sizes[3][2] = {{16, 12}, {38, 26}, {12, 80}};
    const int thrs[4] = {1, 64, 255, 1021};
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1], cw = w / 2, ch = h / 2;
        // nearly flat planes: every valid neighbour passes at the larger strengths, so a weight of 0 there is an invalid cell
        std::vector<uint8_t> cur((size_t)w * h), prev((size_t)w * h), next((size_t)w * h);
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
                        qp[2 * c] = sat16(edge_target(k, w) - 8 * cx);
                        qp[2 * c + 1] = variant & 1 ? sat16(edge_target(k / 3 + variant, h) - 8 * cy) : 0;
                        qn[2 * c] = variant & 2 ? sat16(edge_target(k + 5, w) - 8 * cx) : 0;
                        qn[2 * c + 1] = sat16(edge_target(k / 2 + 1, h) - 8 * cy);
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
                    std::vector<uint8_t> out((size_t)w * h, FILL8), map((size_t)cw * ch, FILL8);
                    std::vector<u64> st(4, FILL64);
                    CHECK(bbme_subpel_temporal_filter_host(P, cur.data(), N, w, h, QP, QN, thr, nullptr, out.data(), map.data(),
                                                           st.data()) == BBME_OK);
                    u64 np = 0, nn = 0, ws = 0;
                    for (int cy = 0; cy < ch; ++cy)
                        for (int cx = 0; cx < cw; ++cx) {
                            const size_t c = (size_t)cy * cw + cx;
                            const int wp = map[c] & 15, wn = map[c] >> 4;
                            CHECK(wp <= 8 && wn <= 8);
                            np += wp > 0; nn += wn > 0; ws += (u64)(wp + wn);
                            const bool vp = P && inside(8 * cx + qp[2 * c], w) && inside(8 * cy + qp[2 * c + 1], h);
                            const bool vn = N && inside(8 * cx + qn[2 * c], w) && inside(8 * cy + qn[2 * c + 1], h);
                            if (!vp) CHECK(wp == 0);
                            if (!vn) CHECK(wn == 0);
                            if (thr >= 64) CHECK((wp > 0) == vp && (wn > 0) == vn);       // flat planes: cost <= 12
                            if (!wp && !wn)
                                for (int i = 0; i < 2; ++i)
                                    for (int j = 0; j < 2; ++j)
                                        CHECK(out[(size_t)(2 * cy + i) * w + 2 * cx + j] == cur[(size_t)(2 * cy + i) * w + 2 * cx + j]);
                        }
                    CHECK(st[0] == np && st[1] == nn && st[2] == ws && st[3] <= 1020ull * cw * ch);
                    if (variant == 5) CHECK(np == 0 && nn == 0 && out == cur);
                    if (variant == 4 && thr >= 64) CHECK(np + nn > 0);
                    // each output alone gives the same bytes
                    std::vector<uint8_t> out2((size_t)w * h, FILL8), map2((size_t)cw * ch, FILL8);
                    std::vector<u64> st2(4, FILL64);
                    CHECK(bbme_subpel_temporal_filter_host(P, cur.data(), N, w, h, QP, QN, thr, nullptr, out2.data(), nullptr, nullptr) == BBME_OK);
                    CHECK(bbme_subpel_temporal_filter_host(P, cur.data(), N, w, h, QP, QN, thr, nullptr, nullptr, map2.data(), nullptr) == BBME_OK);
                    CHECK(bbme_subpel_temporal_filter_host(P, cur.data(), N, w, h, QP, QN, thr, nullptr, nullptr, nullptr, st2.data()) == BBME_OK);
                    CHECK(out2 == out && map2 == map && st2 == st);
                    // windows: 1x1 at each corner counts that cell; illegal ones fail and write nothing
                    const int corners[4][2] = {{0, 0}, {cw - 1, 0}, {0, ch - 1}, {cw - 1, ch - 1}};
                    for (const auto &cn : corners) {
                        const int win[4] = {cn[0], cn[1], 1, 1};
                        std::vector<u64> s1(4, FILL64);
                        CHECK(bbme_subpel_temporal_filter_host(P, cur.data(), N, w, h, QP, QN, thr, win, nullptr, nullptr, s1.data()) == BBME_OK);
                        const uint8_t m = map[(size_t)cn[1] * cw + cn[0]];
                        CHECK(s1[0] == (u64)((m & 15) > 0) && s1[1] == (u64)((m >> 4) > 0) && s1[2] == (u64)((m & 15) + (m >> 4)) && s1[3] <= 1020);
                    }
                    const int bad[4][4] = {{-1, 0, 1, 1}, {0, 0, cw + 1, 1}, {0, ch, 1, 1}, {0, 0, 1, 0}};
                    for (const auto &win : bad) {
                        std::vector<uint8_t> o((size_t)w * h, FILL8);
                        std::vector<u64> s1(4, FILL64);
                        CHECK(bbme_subpel_temporal_filter_host(P, cur.data(), N, w, h, QP, QN, thr, win, o.data(), nullptr, s1.data()) ==
                              BBME_ERR_INVALID);
                        for (uint8_t x : o) CHECK(x == FILL8);
                        for (u64 x : s1) CHECK(x == FILL64);
                    }
                }
        }
    }
    printf("subpel temporal filter host rule ok\n");
    return 0;
}
