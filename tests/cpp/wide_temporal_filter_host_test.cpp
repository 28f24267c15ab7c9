// bbme_compose_host and bbme_wide_temporal_filter_host (csrc/bbme_host.cpp, the references of the GPU tests of the CELL COMPOSITION
// RULE and the WIDE TEMPORAL FILTER RULE) under AddressSanitizer and UBSan, as a program of its own: grids, planes and every output
// are exactly sized vectors, so a gather outside a grid, a tap of weight 0 read outside a plane or a value written outside an
// output is a finding.  The composition gets targets outside the grid on every side, ties, int16 extremes and sums that saturate,
// at both unit shifts and with row pitches beyond the row; the filter gets s on and past every edge by a quarter pel and a pixel,
// far outside and on the int16 extremes, for each of the 15 neighbour sets; windows: none, 1x1 at each corner, and illegal ones,
// which must fail and write nothing.  Last, the multiply-shift the kernel divides by S with is proven exact for every numerator
// 0 .. 10220 at every S = 8 .. 40.
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

static uint32_t g_seed = 2026;
static int rnd(int n) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (uint32_t)n); }

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

static int floor_div(int v, int d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }

static void test_compose()
{
    const int sizes[4][2] = {{1, 1}, {5, 3}, {9, 7}, {18, 14}};
    const int16_t ext[4] = {-32768, 32767, -32767, 32766};
    for (const auto &sz : sizes)
        for (int u = 0; u <= 2; u += 2)
            for (int variant = 0; variant < 4; ++variant) {
                const int cw = sz[0], ch = sz[1], unit = 1 << u;
                const int pa = cw + variant, pb = cw + (variant & 1), po = cw + 2 * (variant >> 1);      // pitches beyond the row
                // exactly sized: the last row ends with its last cell
                std::vector<int16_t> a(2 * ((size_t)pa * (ch - 1) + cw)), b(2 * ((size_t)pb * (ch - 1) + cw));
                for (int cy = 0; cy < ch; ++cy)
                    for (int cx = 0; cx < cw; ++cx) {
                        int16_t *va = &a[2 * ((size_t)cy * pa + cx)], *vb = &b[2 * ((size_t)cy * pb + cx)];
                        const int kind = rnd(5);
                        for (int i = 0; i < 2; ++i) {
                            const int n = i ? ch : cw, c = i ? cy : cx;
                            if (kind == 0) va[i] = (int16_t)((rnd(13) - 6) * unit);
                            else if (kind == 1) va[i] = sat16((rnd(6 * n + 1) - 3 * n) * 2 * unit);                   // outside on either side
                            else if (kind == 2) va[i] = sat16((rnd(n + 2) - 1 - c) * 2 * unit + unit - rnd(2));       // ties and one short
                            else if (kind == 3) va[i] = ext[rnd(4)];
                            else va[i] = 0;
                            vb[i] = rnd(3) ? (int16_t)(rnd(2001) - 1000) : ext[rnd(4)];
                        }
                    }
                std::vector<int16_t> out(2 * ((size_t)po * (ch - 1) + cw), (int16_t)FILL16);
                std::vector<u64> st(2, FILL64);
                CHECK(bbme_compose_host(a.data(), pa, b.data(), pb, cw, ch, u, nullptr, out.data(), po, st.data()) == BBME_OK);
                u64 nclamp = 0, nsat = 0;
                for (int cy = 0; cy < ch; ++cy)
                    for (int cx = 0; cx < cw; ++cx) {
                        const int16_t *va = &a[2 * ((size_t)cy * pa + cx)];
                        const int px = floor_div(2 * cx * unit + va[0] + unit, 2 * unit), py = floor_div(2 * cy * unit + va[1] + unit, 2 * unit);
                        const int qx = px < 0 ? 0 : px > cw - 1 ? cw - 1 : px, qy = py < 0 ? 0 : py > ch - 1 ? ch - 1 : py;
                        const int16_t *vb = &b[2 * ((size_t)qy * pb + qx)];
                        const int sx = va[0] + vb[0], sy = va[1] + vb[1];
                        CHECK(out[2 * ((size_t)cy * po + cx)] == sat16(sx) && out[2 * ((size_t)cy * po + cx) + 1] == sat16(sy));
                        nclamp += qx != px || qy != py;
                        nsat += sat16(sx) != sx || sat16(sy) != sy;
                        for (int x = cw; x < po && cy + 1 < ch; ++x) CHECK(out[2 * ((size_t)cy * po + x)] == (int16_t)FILL16);      // the pitch's slack
                    }
                CHECK(st[0] == nclamp && st[1] == nsat);
                // each output alone; B = 0 gives A
                std::vector<int16_t> out2(out.size(), (int16_t)FILL16);
                std::vector<u64> st2(2, FILL64);
                CHECK(bbme_compose_host(a.data(), pa, b.data(), pb, cw, ch, u, nullptr, out2.data(), po, nullptr) == BBME_OK);
                CHECK(bbme_compose_host(a.data(), pa, b.data(), pb, cw, ch, u, nullptr, nullptr, 0, st2.data()) == BBME_OK);
                CHECK(out2 == out && st2 == st);
                std::vector<int16_t> zero(b.size(), 0);
                CHECK(bbme_compose_host(a.data(), pa, zero.data(), pb, cw, ch, u, nullptr, out2.data(), po, nullptr) == BBME_OK);
                for (int cy = 0; cy < ch; ++cy)
                    for (int cx = 0; cx < 2 * cw; ++cx) CHECK(out2[2 * (size_t)cy * po + cx] == a[2 * (size_t)cy * pa + cx]);
                const int win[4] = {cw - 1, ch - 1, 1, 1}, bad[4] = {0, 0, cw + 1, 1};
                CHECK(bbme_compose_host(a.data(), pa, b.data(), pb, cw, ch, u, win, nullptr, 0, st2.data()) == BBME_OK);
                CHECK(st2[0] <= 1 && st2[1] <= 1);
                std::vector<u64> st3(2, FILL64);
                CHECK(bbme_compose_host(a.data(), pa, b.data(), pb, cw, ch, u, bad, out2.data(), po, st3.data()) == BBME_ERR_INVALID);
                CHECK(st3[0] == FILL64 && st3[1] == FILL64);
            }
}

static void test_wide_filter()
{
    const int sizes[3][2] = {{16, 12}, {38, 26}, {12, 80}};
    const int thrs[3] = {1, 64, 1021};
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1], cw = w / 2, ch = h / 2;
        // nearly flat planes: every valid neighbour passes at the larger strengths, so a weight of 0 there is an invalid cell
        std::vector<uint8_t> cur((size_t)w * h), nb[4];
        for (auto &x : cur) x = (uint8_t)(100 + rnd(4));
        for (auto &p : nb) { p.resize((size_t)w * h); for (auto &x : p) x = (uint8_t)(100 + rnd(4)); }
        for (int variant = 0; variant < 4; ++variant) {
            const int pitch = cw + (variant & 1) * 3;
            std::vector<int16_t> q[4];
            for (int k = 0; k < 4; ++k) {
                q[k].assign(2 * ((size_t)pitch * (ch - 1) + cw), 0);
                for (int cy = 0; cy < ch; ++cy)
                    for (int cx = 0; cx < cw; ++cx) {
                        int16_t *v = &q[k][2 * ((size_t)cy * pitch + cx)];
                        const int c = cy * cw + cx + 3 * variant + 5 * k;
                        if (variant < 2) {                     // one axis on an edge position, the other in place or on one too
                            v[0] = sat16(edge_target(c, w) - 8 * cx);
                            v[1] = (variant + k) & 1 ? sat16(edge_target(c / 3 + k, h) - 8 * cy) : 0;
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
                    const uint8_t *planes[4];
                    const int16_t *grids[4];
                    for (int k = 0; k < 4; ++k) {
                        planes[k] = set >> k & 1 ? nb[k].data() : nullptr;
                        grids[k] = set >> k & 1 ? q[k].data() : nullptr;
                    }
                    std::vector<uint8_t> out((size_t)w * h, FILL8);
                    std::vector<uint16_t> map((size_t)cw * ch, FILL16);
                    std::vector<u64> st(6, FILL64);
                    CHECK(bbme_wide_temporal_filter_host(planes, cur.data(), w, h, grids, pitch, thr, nullptr, out.data(), map.data(),
                                                         st.data()) == BBME_OK);
                    u64 n[4] = {0, 0, 0, 0}, ws = 0;
                    for (int cy = 0; cy < ch; ++cy)
                        for (int cx = 0; cx < cw; ++cx) {
                            const uint16_t m = map[(size_t)cy * cw + cx];
                            int sum = 0;
                            for (int k = 0; k < 4; ++k) {
                                const int wk = m >> (4 * k) & 15;
                                CHECK(wk <= 8);
                                const int16_t *v = &q[k][2 * ((size_t)cy * pitch + cx)];
                                const bool valid = planes[k] && inside(8 * cx + v[0], w) && inside(8 * cy + v[1], h);
                                if (!valid) CHECK(wk == 0);
                                if (thr >= 64) CHECK((wk > 0) == valid);               // flat planes: cost <= 12
                                n[k] += wk > 0; sum += wk;
                            }
                            ws += (u64)sum;
                            if (!sum)
                                for (int i = 0; i < 2; ++i)
                                    for (int j = 0; j < 2; ++j)
                                        CHECK(out[(size_t)(2 * cy + i) * w + 2 * cx + j] == cur[(size_t)(2 * cy + i) * w + 2 * cx + j]);
                        }
                    CHECK(st[0] == n[0] && st[1] == n[1] && st[2] == n[2] && st[3] == n[3] && st[4] == ws && st[5] <= 1020ull * cw * ch);
                    if (variant == 3) CHECK(ws == 0 && out == cur);
                    if (variant == 2 && thr >= 64) CHECK(ws > 0);
                    // each output alone gives the same bytes
                    std::vector<uint8_t> out2((size_t)w * h, FILL8);
                    std::vector<uint16_t> map2((size_t)cw * ch, FILL16);
                    std::vector<u64> st2(6, FILL64);
                    CHECK(bbme_wide_temporal_filter_host(planes, cur.data(), w, h, grids, pitch, thr, nullptr, out2.data(), nullptr, nullptr) == BBME_OK);
                    CHECK(bbme_wide_temporal_filter_host(planes, cur.data(), w, h, grids, pitch, thr, nullptr, nullptr, map2.data(), nullptr) == BBME_OK);
                    CHECK(bbme_wide_temporal_filter_host(planes, cur.data(), w, h, grids, pitch, thr, nullptr, nullptr, nullptr, st2.data()) == BBME_OK);
                    CHECK(out2 == out && map2 == map && st2 == st);
                    if (set % 5) continue;                     // windows on a third of the sets
                    const int corners[4][2] = {{0, 0}, {cw - 1, 0}, {0, ch - 1}, {cw - 1, ch - 1}};
                    for (const auto &cn : corners) {
                        const int win[4] = {cn[0], cn[1], 1, 1};
                        std::vector<u64> s1(6, FILL64);
                        CHECK(bbme_wide_temporal_filter_host(planes, cur.data(), w, h, grids, pitch, thr, win, nullptr, nullptr, s1.data()) == BBME_OK);
                        const uint16_t m = map[(size_t)cn[1] * cw + cn[0]];
                        u64 sum = 0;
                        for (int k = 0; k < 4; ++k) { CHECK(s1[k] == (u64)((m >> (4 * k) & 15) > 0)); sum += m >> (4 * k) & 15; }
                        CHECK(s1[4] == sum && s1[5] <= 1020);
                    }
                    const int bad[4][4] = {{-1, 0, 1, 1}, {0, 0, cw + 1, 1}, {0, ch, 1, 1}, {0, 0, 1, 0}};
                    for (const auto &win : bad) {
                        std::vector<uint8_t> o((size_t)w * h, FILL8);
                        std::vector<u64> s1(6, FILL64);
                        CHECK(bbme_wide_temporal_filter_host(planes, cur.data(), w, h, grids, pitch, thr, win, o.data(), nullptr, s1.data()) ==
                              BBME_ERR_INVALID);
                        for (uint8_t x : o) CHECK(x == FILL8);
                        for (u64 x : s1) CHECK(x == FILL64);
                    }
                }
        }
    }
}

// umulhi(n, floor(2^32 / S) + 1) = n / S for every numerator the blend can have, at every S
static void test_division_by_the_weight_sum()
{
    for (uint32_t S = 8; S <= 40; ++S) {
        const uint32_t magic = (uint32_t)((1ull << 32) / S + 1ull);
        for (uint32_t n = 0; n <= 255u * 40u + 20u; ++n) CHECK((uint32_t)(((u64)n * magic) >> 32) == n / S);
    }
}

int main()
{
    test_compose();
    test_wide_filter();
    test_division_by_the_weight_sum();
    printf("wide temporal filter host rules ok\n");
    return 0;
}
