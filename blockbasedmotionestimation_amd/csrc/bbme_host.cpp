// bbme_host.cpp -- host side of libbbme.so: everything of the drop-in boundary that the
// reference also does on the CPU.  MF::MF's padding + pyramid (motion_framework.cpp:4-111),
// the spiral visiting order (:326-411) as a table, and the Flow class' .flo codec and EPE
// (rw_flow.cpp:39-200,309-332).  No GPU code here; no dependency on oracle/.
#include "bbme_internal.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <set>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <unistd.h>

namespace bbme {

// ---------------------------------------------------------------------------------------
// error channel
// ---------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int fail(int status, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return status;
}

void clear_error() { g_last_error.clear(); }

static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int validate_params(const bbme_params &p)
{
    if (p.num_levels <= 0 || p.num_levels > BBME_MAX_LEVELS)      // assert(num_levels > 0), :7
        return fail(BBME_ERR_INVALID, "num_levels must be in 1..%d (got %d)", BBME_MAX_LEVELS, p.num_levels);
    for (int i = 0; i < p.num_levels; ++i) {
        if (!is_pow2(p.block_size[i]) || p.block_size[i] < 2 || p.block_size[i] > 64)
            return fail(BBME_ERR_UNSUPPORTED,
                        "block_size[%d]=%d: the kernels need a power of two in 2..64 "
                        "(the regulariser halves blocks down to 2x2)", i, p.block_size[i]);
        if (p.search_size[i] <= 0)
            return fail(BBME_ERR_INVALID, "search_size[%d]=%d must be positive", i, p.search_size[i]);
        int range = (p.search_size[i] - p.block_size[i]) >> 1;
        // (ranks of the spiral walk are 16-bit: (2 * 127 + 1)^2 - 1 < 0xffff.  Ranges up to 63 take the strip kernel where the block
        // size allows, larger ones the generic kernel)
        if (range > 127)
            return fail(BBME_ERR_UNSUPPORTED, "search range %d at level %d exceeds 127", range, i);
    }
    return BBME_OK;
}

// ---------------------------------------------------------------------------------------
// Padding search (motion_framework.cpp:14-54).  The reference grows height and width one
// pixel at a time until both are divisible by 2^i * block_size[i] for every level, and
// gives up when either reaches twice the original.  Each dimension therefore ends at the
// next multiple of M = lcm_i(2^i * block_size[i]); reaching 2x the original is an error.
// ---------------------------------------------------------------------------------------
int plan_padding(int width, int height, const bbme_params &p, Geometry &g)
{
    if (width <= 0 || height <= 0)
        return fail(BBME_ERR_INVALID, "frame size %dx%d is not positive", width, height);
    long long m = 1;
    for (int i = 0; i < p.num_levels; ++i)
        m = std::lcm(m, (long long)p.block_size[i] << i);
    long long th = ((height + m - 1) / m) * m, tw = ((width + m - 1) / m) * m;
    if (th >= 2LL * height || tw >= 2LL * width)
        return fail(BBME_ERR_PADDING,
                    "Could not find any multiples of the block size that match padded image dimensions "
                    "(%dx%d, need multiples of %lld)", width, height, m);
    if ((th - height) % 2 != 0 || (tw - width) % 2 != 0)
        return fail(BBME_ERR_ODD_PADDING,
                    "padded size %lldx%lld differs from %dx%d by an odd amount: the reference would "
                    "allocate a mis-sized image (motion_framework.cpp:50-58)", tw, th, width, height);
    g.width = width; g.height = height;
    g.padded_width = (int)tw; g.padded_height = (int)th;
    g.pad_x = (int)(tw - width) / 2; g.pad_y = (int)(th - height) / 2;
    return BBME_OK;
}

void pad_zero(const uint8_t *src, int width, int height, int pitch, int pad_x, int pad_y, uint8_t *dst)
{
    const int pw = width + 2 * pad_x;
    uint8_t *out = dst;
    for (int y = 0; y < pad_y; ++y, out += pw) memset(out, 0, (size_t)pw);
    for (int y = 0; y < height; ++y, out += pw) {
        memset(out, 0, (size_t)pad_x);
        memcpy(out + pad_x, src + (size_t)y * pitch, (size_t)width);
        memset(out + pad_x + width, 0, (size_t)pad_x);
    }
    for (int y = 0; y < pad_y; ++y, out += pw) memset(out, 0, (size_t)pw);
}

// cv::pyrDown on 8-bit data (motion_framework.cpp:89-90): 5x5 binomial [1 4 6 4 1]^2 / 256,
// integer with one rounding (+128 >> 8), BORDER_REFLECT_101, destination pixel (x,y) centred on
// source (2x,2y).  Horizontal sums of the five source rows of a destination row are kept in a
// ring so every source row is filtered once.
static inline int mirror101(int p, int n)
{
    if (n == 1) return 0;
    for (;;) {
        if (p < 0) p = -p;
        else if (p >= n) p = 2 * n - 2 - p;
        else return p;
    }
}

void pyr_down(const uint8_t *src, int sw, int sh, uint8_t *dst)
{
    const int dw = sw / 2, dh = sh / 2;
    std::vector<int> hsum((size_t)sh * dw);
    std::vector<int> xm((size_t)dw * 5);
    for (int x = 0; x < dw; ++x)
        for (int t = 0; t < 5; ++t) xm[(size_t)x * 5 + t] = mirror101(2 * x + t - 2, sw);
    for (int y = 0; y < sh; ++y) {
        const uint8_t *s = src + (size_t)y * sw;
        int *h = &hsum[(size_t)y * dw];
        for (int x = 0; x < dw; ++x) {
            const int *m = &xm[(size_t)x * 5];
            h[x] = s[m[0]] + 4 * s[m[1]] + 6 * s[m[2]] + 4 * s[m[3]] + s[m[4]];
        }
    }
    for (int y = 0; y < dh; ++y) {
        const int *r0 = &hsum[(size_t)mirror101(2 * y - 2, sh) * dw];
        const int *r1 = &hsum[(size_t)mirror101(2 * y - 1, sh) * dw];
        const int *r2 = &hsum[(size_t)mirror101(2 * y, sh) * dw];
        const int *r3 = &hsum[(size_t)mirror101(2 * y + 1, sh) * dw];
        const int *r4 = &hsum[(size_t)mirror101(2 * y + 2, sh) * dw];
        uint8_t *d = dst + (size_t)y * dw;
        for (int x = 0; x < dw; ++x)
            d[x] = (uint8_t)((r0[x] + 4 * r1[x] + 6 * r2[x] + 4 * r3[x] + r4[x] + 128) >> 8);
    }
}

// cv::resize(img, img, Size(), 4, 4, INTER_LINEAR) on 8-bit data (main_class.cpp:32-33):
// OpenCV's fixed-point bilinear -- 11-bit coefficients, horizontal pass to int, vertical pass
// ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2) >> 2.
void resize_x4(const uint8_t *src, int sw, int sh, uint8_t *dst)
{
    const int dw = sw * 4, dh = sh * 4;
    auto coef = [](float f) {
        long r = lrintf(f * 2048.f);
        return (short)(r > 32767 ? 32767 : (r < -32768 ? -32768 : r));
    };
    std::vector<int> sx0(dw), sx1(dw);
    std::vector<short> ax0(dw), ax1(dw);
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * 0.25 - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { sx = 0; fx = 0; }
        if (sx >= sw - 1) { sx = sw - 1; fx = 0; }
        sx0[dx] = sx;
        sx1[dx] = sx + 1 < sw ? sx + 1 : sx;       // weight is 0 there
        ax0[dx] = coef(1.f - fx);
        ax1[dx] = coef(fx);
        if (sx + 1 >= sw) { ax0[dx] = 2048; ax1[dx] = 0; }
    }
    std::vector<int> row0(dw), row1(dw);
    int have0 = -1, have1 = -1;
    auto hpass = [&](int sy, std::vector<int> &out) {
        const uint8_t *s = src + (size_t)sy * sw;
        for (int dx = 0; dx < dw; ++dx) out[dx] = s[sx0[dx]] * ax0[dx] + s[sx1[dx]] * ax1[dx];
    };
    for (int dy = 0; dy < dh; ++dy) {
        float fy = (float)((dy + 0.5) * 0.25 - 0.5);
        int sy = (int)floorf(fy);
        fy -= sy;
        int b0 = coef(1.f - fy), b1 = coef(fy);
        int y0 = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
        int y1 = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
        if (have0 != y0) {
            if (have1 == y0) { row0.swap(row1); std::swap(have0, have1); }
            else { hpass(y0, row0); have0 = y0; }
        }
        if (have1 != y1) { hpass(y1, row1); have1 = y1; }
        uint8_t *d = dst + (size_t)dy * dw;
        for (int dx = 0; dx < dw; ++dx)
            d[dx] = (uint8_t)((((b0 * (row0[dx] >> 4)) >> 16) + ((b1 * (row1[dx] >> 4)) >> 16) + 2) >> 2);
    }
}

// ---------------------------------------------------------------------------------------
// Spiral order (motion_framework.cpp:326-411): centre; then for m = 1,3,5,... < shift:
// right m, down m, left m+1, up m+1; finally right m-1.  Walked literally.
// ---------------------------------------------------------------------------------------
SpiralTable build_spiral(int search_size, int block_size)
{
    SpiralTable t;
    const int shift = search_size - block_size;
    int l = 0, k = 0, m, s;
    auto emit = [&]() { t.dx.push_back((int16_t)l); t.dy.push_back((int16_t)k); };
    emit();
    for (m = 1; m < shift; m += 2) {
        for (s = 0; s < m; ++s) { ++l; emit(); }
        for (s = 0; s < m; ++s) { ++k; emit(); }
        for (s = 0; s < m + 1; ++s) { --l; emit(); }
        for (s = 0; s < m + 1; ++s) { --k; emit(); }
    }
    for (s = 0; s < m - 1; ++s) { ++l; emit(); }
    int r = 0;
    for (size_t i = 0; i < t.dx.size(); ++i) {
        r = std::max(r, std::abs((int)t.dx[i]));
        r = std::max(r, std::abs((int)t.dy[i]));
    }
    t.range = r;
    t.side = 2 * r + 1;
    t.rank_pitch = (t.side + 3) & ~3;
    t.rank_of.assign((size_t)t.rank_pitch * t.side, 0xFFFF);
    for (size_t i = 0; i < t.dx.size(); ++i)
        t.rank_of[(size_t)(t.dy[i] + r) * t.rank_pitch + (t.dx[i] + r)] = (uint16_t)i;
    return t;
}

// ---------------------------------------------------------------------------------------
// Work split of k_search_fast.  Every (column group, candidate row) pair must be covered exactly
// once.  A round costs its strip height whatever the number of busy lanes, so rounds are kept
// full: take the tallest strip height that still has 64 strips available; what is left (< 64
// single rows) goes into one last round of height 1.
// ---------------------------------------------------------------------------------------
SearchPlan plan_search(int range, int block_size, int max_strip, int lanes, bool loose)
{
    SearchPlan p;
    const int n = 2 * range + 1;
    p.groups = (n + 3) / 4;
    p.pitch_dw = (p.groups + block_size / 4) | 1;
    // n = 4 G' + 1 (every even range): the last column group would hold ONE candidate column and three of padding, and
    // the last candidate row a strip of height one in every group -- 9 % of the QSADs of a +-32 search.  The tight plan
    // packs the G' x (n - 1) rectangle into strips and gives the rim its own rounds (kernel: search_row_parts,
    // search_aligned_column): kind 1, candidate row n - 1 of the G' full groups, four lanes per (group, row), a quarter of
    // the block's rows each; kind 2, candidate column n - 1 (dx = +R, dword aligned in the staged window: R is even),
    // one candidate per lane, v_sad_u8.  rounds[] = S | kind << 8.
    const bool tight = n % 4 == 1 && n >= 9 && block_size <= 16 && !loose;
    const int groups_main = tight ? p.groups - 1 : p.groups, rows_main = tight ? n - 1 : n;
    std::vector<int> next(groups_main, 0);                   // first uncovered candidate row per column group
    auto emit_round = [&](int s, int want) {
        p.rounds.push_back((uint32_t)s);
        std::vector<uint32_t> t;
        // strips row by row of columns: lane = strip_row * groups + g keeps a round's LDS reads spread
        bool more = true;
        while (more && (int)t.size() < want) {
            more = false;
            for (int g = 0; g < groups_main && (int)t.size() < want; ++g)
                if (rows_main - next[g] >= s) {
                    t.push_back((uint32_t)g | ((uint32_t)next[g] << 8));
                    next[g] += s;
                    more = true;
                }
        }
        t.resize((size_t)((t.size() + lanes - 1) / lanes * lanes), 0xffffffffu);   // whole rounds of `lanes` tasks
        p.tasks.insert(p.tasks.end(), t.begin(), t.end());
    };
    for (int s = max_strip; s >= 1; s >>= 1) {
        for (;;) {
            int avail = 0;
            for (int g = 0; g < groups_main; ++g) avail += (rows_main - next[g]) / s;
            if (avail >= lanes) emit_round(s, lanes);
            else break;
        }
    }
    int left = 0;
    for (int g = 0; g < groups_main; ++g) left += rows_main - next[g];
    while (left > 0) { emit_round(1, std::min(left, lanes)); left -= std::min(left, lanes); }
    if (tight) {
        auto emit_tasks = [&](uint32_t kind, const std::vector<uint32_t> &all) {
            for (size_t i = 0; i < all.size(); i += (size_t)lanes) {
                p.rounds.push_back(1u | kind << 8);
                for (int k = 0; k < lanes; ++k)
                    p.tasks.push_back(i + k < all.size() ? all[i + k] : 0xffffffffu);
            }
        };
        std::vector<uint32_t> parts, column;
        for (int g = 0; g < groups_main; ++g)
            for (uint32_t part = 0; part < 4; ++part)       // the four lanes of a quad share one (group, row)
                parts.push_back((uint32_t)g | (uint32_t)(n - 1) << 8 | part << 16);
        for (int dy = 0; dy < n; ++dy) column.push_back((uint32_t)dy);
        emit_tasks(1u, parts);
        emit_tasks(2u, column);
    }
    return p;
}

// ---------------------------------------------------------------------------------------
// Flow::ReadFlowFile / WriteFlowFile / CalculateMSE (rw_flow.cpp)
// ---------------------------------------------------------------------------------------
static const float kTagFloat = 202021.25f;      // rw_flow.cpp:25
static const char kTagString[] = "PIEH";        // rw_flow.cpp:26

int flo_read(const char *filename, int *width, int *height, float **data)
{
    if (!filename) return fail(BBME_ERR_IO, "ReadFlowFile: empty filename");
    const char *dot = strrchr(filename, '.');
    if (!dot || strcmp(dot, ".flo") != 0)
        return fail(BBME_ERR_IO, "ReadFlowFile extension .flo expected");
    FILE *f = fopen(filename, "rb");
    if (!f) return fail(BBME_ERR_IO, "ReadFlowFile: could not open file %s", filename);
    float tag; int w, h;
    if (fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1) {
        fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: problem reading file");
    }
    if (tag != kTagFloat) { fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: wrong tag (possibly due to big-endian machine?)"); }
    if (w < 1 || w > 99999) { fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: illegal width %d", w); }
    if (h < 1 || h > 99999) { fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: illegal height %d", h); }
    const size_t n = (size_t)w * h * 2;
    float *buf = (float *)malloc(n * sizeof(float));
    if (!buf) { fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: out of memory"); }
    if (fread(buf, sizeof(float), n, f) != n) { free(buf); fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: file is too short"); }
    if (fgetc(f) != EOF) { free(buf); fclose(f); return fail(BBME_ERR_IO, "ReadFlowFile: file is too long"); }
    fclose(f);
    *width = w; *height = h; *data = buf;
    return BBME_OK;
}

int flo_write(const char *filename, int width, int height, const float *data)
{
    if (!filename) return fail(BBME_ERR_IO, "WriteFlowFile: empty filename");
    const char *dot = strrchr(filename, '.');
    if (!dot) return fail(BBME_ERR_IO, "WriteFlowFile: extension required in filename");
    if (strcmp(dot, ".flo") != 0) return fail(BBME_ERR_IO, "WriteFlowFile: filename should have extension '.flo'");
    if (width < 1 || height < 1 || !data) return fail(BBME_ERR_INVALID, "WriteFlowFile: empty image");
    FILE *f = fopen(filename, "wb");
    if (!f) return fail(BBME_ERR_IO, "WriteFlowFile: could not open file %s", filename);
    const size_t n = (size_t)width * height * 2;
    bool ok = fwrite(kTagString, 1, 4, f) == 4 && fwrite(&width, 4, 1, f) == 1 && fwrite(&height, 4, 1, f) == 1;
    ok = ok && fwrite(data, sizeof(float), n, f) == n;
    ok = (fclose(f) == 0) && ok;
    return ok ? BBME_OK : fail(BBME_ERR_IO, "WriteFlowFile: problem writing data");
}

static inline bool unknown_flow(float u, float v)
{
    return std::fabs(u) > 1e9 || std::fabs(v) > 1e9 || std::isnan(u) || std::isnan(v);
}

double calculate_mse(const float *gtruth, const float *flow, int width, int height)
{
    long long count = 0;
    double error = 0;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) {
        const float gu = gtruth[2 * i], gv = gtruth[2 * i + 1];
        if (unknown_flow(gu, gv)) continue;
        ++count;
        const float du = gu - flow[2 * i], dv = gv - flow[2 * i + 1];
        const float sq = du * du + dv * dv;     // float arithmetic as the reference's expression
        error += std::sqrt(sq);
    }
    return error / (double)count;
}

// ---- Flow::MotionToColor / computeColor / makecolorwheel (rw_flow.cpp:202-307) -------------
// The Middlebury colour wheel: 55 hues in six transitions whose lengths follow perceptual
// similarity.  Entry k of a transition of length n from colour A towards B moves one channel
// by 255*i/n (integer division), exactly as the reference's six loops do.
namespace {
struct ColorWheel {
    static constexpr int kCols = 15 + 6 + 4 + 11 + 13 + 6;
    int rgb[kCols][3];
    ColorWheel()
    {
        static const int len[6] = {15, 6, 4, 11, 13, 6};          // RY YG GC CB BM MR
        static const int moving[6] = {1, 0, 2, 1, 0, 2};          // channel that changes
        static const int rising[6] = {1, 0, 1, 0, 1, 0};          // ... upwards or downwards
        static const int base[6][3] = {{255, 0, 0}, {255, 255, 0}, {0, 255, 0}, {0, 255, 255}, {0, 0, 255}, {255, 0, 255}};
        int k = 0;
        for (int t = 0; t < 6; ++t)
            for (int i = 0; i < len[t]; ++i, ++k) {
                for (int c = 0; c < 3; ++c) rgb[k][c] = base[t][c];
                const int step = 255 * i / len[t];
                rgb[k][moving[t]] = rising[t] ? step : 255 - step;
            }
    }
};
const ColorWheel g_wheel;

// computeColor (rw_flow.cpp:251-275): hue from the angle, saturation from the radius; all float
// except the division by pi and the final scaling, which the reference's expressions do in double.
inline void compute_color(float fx, float fy, uint8_t *bgr)
{
    const int ncols = ColorWheel::kCols;
    const float rad = std::sqrt(fx * fx + fy * fy);
    const float a = (float)(std::atan2(-fy, -fx) / 3.14159265358979323846);   // M_PI
    const float fk = (a + 1.0f) / 2.0f * (float)(ncols - 1);
    const int k0 = (int)fk;
    const int k1 = (k0 + 1) % ncols;
    const float f = fk - (float)k0;
    for (int b = 0; b < 3; ++b) {
        const float col0 = (float)g_wheel.rgb[k0][b] / 255.0f;
        const float col1 = (float)g_wheel.rgb[k1][b] / 255.0f;
        float col = (1 - f) * col0 + f * col1;
        if (rad <= 1) col = 1 - rad * (1 - col);               // increase saturation with radius
        else col = (float)(col * .75);                          // out of range
        bgr[2 - b] = (uint8_t)(int)(255.0 * col);
    }
}
}  // namespace

void motion_to_color(const float *flow, int width, int height, float maxmotion, uint8_t *bgr, float range[5])
{
    float maxx = -999, maxy = -999, minx = 999, miny = 999, maxrad = -1;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) {
        const float fx = flow[2 * i], fy = flow[2 * i + 1];
        if (unknown_flow(fx, fy)) continue;
        maxx = maxx > fx ? maxx : fx;
        maxy = maxy > fy ? maxy : fy;
        minx = minx < fx ? minx : fx;
        miny = miny < fy ? miny : fy;
        const float rad = std::sqrt(fx * fx + fy * fy);
        maxrad = maxrad > rad ? maxrad : rad;
    }
    if (range) { range[0] = maxrad; range[1] = minx; range[2] = maxx; range[3] = miny; range[4] = maxy; }
    if (maxmotion > 0) maxrad = maxmotion;                      // i.e. specified by the caller
    if (maxrad == 0) maxrad = 1;                                // flow == 0 everywhere
    for (size_t i = 0; i < n; ++i) {
        const float fx = flow[2 * i], fy = flow[2 * i + 1];
        uint8_t *pix = bgr + 3 * i;
        if (unknown_flow(fx, fy)) pix[0] = pix[1] = pix[2] = 0;
        else compute_color(fx / maxrad, fy / maxrad, pix);
    }
}

// The colour rule of include/bbme.h on a 2x2-cell grid: MotionToColor of the field the driver's subsampling makes of the
// grid, with compute_color's expressions except the hue angle, which is the double atan2 rounded to float (what the kernels
// of bbme_kernels.hpp can reproduce; compute_color's float atan2 is whatever the platform's libm makes of it).
void cells_color(const int16_t *cells, int cells_w, int width, int height, int pad_x, int pad_y, int scale, float maxmotion,
                 uint8_t *bgr, float range[5])
{
#pragma clang fp contract(off)
    const int ow = (int)(((long long)width + scale - 1) / scale), oh = (int)(((long long)height + scale - 1) / scale);
    const float s = (float)scale;
    auto cell = [&](int x, int y) { return cells + 2 * ((size_t)((pad_y + scale * y) >> 1) * cells_w + ((pad_x + scale * x) >> 1)); };
    float maxx = -999, maxy = -999, minx = 999, miny = 999, maxrad = -1;
    if (range || !(maxmotion > 0))
        for (int y = 0; y < oh; ++y)
            for (int x = 0; x < ow; ++x) {
                const int16_t *m = cell(x, y);
                const float fx = (float)m[0] / s, fy = (float)m[1] / s;
                maxx = maxx > fx ? maxx : fx;
                maxy = maxy > fy ? maxy : fy;
                minx = minx < fx ? minx : fx;
                miny = miny < fy ? miny : fy;
                const float rad = std::sqrt(fx * fx + fy * fy);
                maxrad = maxrad > rad ? maxrad : rad;
            }
    if (range) { range[0] = maxrad; range[1] = minx; range[2] = maxx; range[3] = miny; range[4] = maxy; }
    if (!bgr) return;
    if (maxmotion > 0) maxrad = maxmotion;
    if (maxrad == 0) maxrad = 1;
    const int ncols = ColorWheel::kCols;
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            const int16_t *m = cell(x, y);
            const float fx = (float)m[0] / s / maxrad, fy = (float)m[1] / s / maxrad;
            const float rad = std::sqrt(fx * fx + fy * fy);
            const float angle = (float)std::atan2((double)-fy, (double)-fx);
            const float a = (float)((double)angle / 3.14159265358979323846);
            const float fk = (a + 1.0f) / 2.0f * (float)(ncols - 1);
            const int k0 = (int)fk;
            const int k1 = (k0 + 1) % ncols;
            const float f = fk - (float)k0;
            uint8_t *pix = bgr + 3 * ((size_t)y * ow + x);
            for (int b = 0; b < 3; ++b) {
                const float col0 = (float)g_wheel.rgb[k0][b] / 255.0f;
                const float col1 = (float)g_wheel.rgb[k1][b] / 255.0f;
                float col = (1 - f) * col0 + f * col1;
                if (rad <= 1) col = 1 - rad * (1 - col);
                else col = (float)(col * .75);
                pix[2 - b] = (uint8_t)(int)(255.0 * col);
            }
        }
}

int ppm_write_bgr(const char *filename, int width, int height, const uint8_t *bgr)
{
    FILE *f = fopen(filename, "wb");
    if (!f) return fail(BBME_ERR_IO, "ppm_write: could not open %s", filename);
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    std::vector<uint8_t> row((size_t)width * 3);
    bool ok = true;
    for (int y = 0; y < height && ok; ++y) {
        const uint8_t *s = bgr + (size_t)y * width * 3;
        for (int x = 0; x < width; ++x) { row[3 * x] = s[3 * x + 2]; row[3 * x + 1] = s[3 * x + 1]; row[3 * x + 2] = s[3 * x]; }
        ok = fwrite(row.data(), 1, row.size(), f) == row.size();
    }
    if (fclose(f) != 0) ok = false;
    return ok ? BBME_OK : fail(BBME_ERR_IO, "ppm_write: problem writing %s", filename);
}

void subsample_div4(const float *flow_padded, int padded_width, int padded_height,
                    int pad_x, int pad_y, float *out, int out_width)
{
    for (int i = pad_y; i < padded_height - pad_y; i += 4)
        for (int j = pad_x; j < padded_width - pad_x; j += 4) {
            const float *s = flow_padded + 2 * ((size_t)i * padded_width + j);
            float *d = out + 2 * ((size_t)((i - pad_y) / 4) * out_width + (j - pad_x) / 4);
            d[0] = s[0] / 4;
            d[1] = s[1] / 4;
        }
}

// The window of a rule's statistics: {x0, y0, w, h} inside limit_w x limit_h cells (or pixels of a plane), null = all of them.
struct CellWindow {
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    // BBME_OK, or BBME_ERR_INVALID "<what>: window not inside the <limit_w>x<limit_h> <unit>"
    int set(const int *window, int limit_w, int limit_h, const char *what, const char *unit)
    {
        if (window && (window[0] < 0 || window[1] < 0 || window[2] < 1 || window[3] < 1 ||
                       (long long)window[0] + window[2] > limit_w || (long long)window[1] + window[3] > limit_h))
            return fail(BBME_ERR_INVALID, "%s: window not inside the %dx%d %s", what, limit_w, limit_h, unit);
        x0 = window ? window[0] : 0;
        y0 = window ? window[1] : 0;
        x1 = window ? window[0] + window[2] : limit_w;
        y1 = window ? window[1] + window[3] : limit_h;
        return BBME_OK;
    }
    bool contains(int x, int y) const { return x >= x0 && x < x1 && y >= y0 && y < y1; }
};

// MF::draw_MVimage (motion_framework.cpp:887-905) as include/bbme.h states it, block by block, with the residual statistics
static void motion_compensate(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *grid, int grid_block,
                              int block, int fill, const CellWindow &win, uint8_t *out, unsigned long long stats[4])
{
    const int gcols = (width + grid_block - 1) / grid_block;
    unsigned long long sse = 0, sad = 0, pixels = 0, skipped = 0;
    for (int Y = 0; Y < height; Y += block)
        for (int X = 0; X < width; X += block) {
            const int16_t *mv = grid + 2 * ((size_t)(Y / grid_block) * gcols + X / grid_block);
            const int sx = X + mv[0], sy = Y + mv[1];
            const bool ok = sx >= 0 && sx <= width - block && sy >= 0 && sy <= height - block;
            for (int i = 0; i < block && Y + i < height; ++i)
                for (int j = 0; j < block && X + j < width; ++j) {
                    const int v = ok ? image2[(size_t)(sy + i) * width + sx + j] : fill;
                    if (out) out[(size_t)(Y + i) * width + X + j] = (uint8_t)v;
                    if (!stats || !win.contains(X + j, Y + i)) continue;
                    if (!ok) { ++skipped; continue; }
                    const int d = v - image1[(size_t)(Y + i) * width + X + j];
                    sse += (unsigned long long)(d * d);
                    sad += (unsigned long long)(d < 0 ? -d : d);
                    ++pixels;
                }
        }
    if (stats) { stats[0] = sse; stats[1] = sad; stats[2] = pixels; stats[3] = skipped; }
}

// Hypothesis k of the interpolation rule at cell (cx, cy) of a grid cw cells wide, for the phase num / den: its vector v (0: the
// forward one, 1: minus the backward one, 2: zero) and where its two 2x2 blocks start -- p1 = the cell's origin - round(num v /
// den) in frame 1, p2 = p1 + v in frame 2.
struct Hypothesis { int vx, vy, p1x, p1y, p2x, p2y; };
static Hypothesis hypothesis(const int16_t *fwd, const int16_t *bwd, int cw, int cx, int cy, int k, int num, int den)
{
    const auto floor_div = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    const size_t c = (size_t)cy * cw + cx;
    Hypothesis h;
    h.vx = k == 0 ? fwd[2 * c] : k == 1 ? -(int)bwd[2 * c] : 0;
    h.vy = k == 0 ? fwd[2 * c + 1] : k == 1 ? -(int)bwd[2 * c + 1] : 0;
    h.p1x = 2 * cx - floor_div(num * h.vx + den / 2, den);
    h.p1y = 2 * cy - floor_div(num * h.vy + den / 2, den);
    h.p2x = h.p1x + h.vx;
    h.p2y = h.p1y + h.vy;
    return h;
}

// The temporal filter rule of include/bbme.h, cell by cell of the padded view, in the header's own words (the mirror of
// k_temporal_filter and k_temporal_filter_bgr), for frames of `chans` interleaved channels: the width x height frame sits at
// (pad_x, pad_y) of the view and reads 0 outside itself; a neighbour's cost is the largest of its channels' 2x2 SADs.  A grey
// plane is one channel without padding (the plane is the view); a B,G,R frame is three.
static void temporal_filter(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int chans, int width, int height, int pad_x,
                            int pad_y, const int16_t *to_prev, const int16_t *to_next, int thr, const CellWindow &win, uint8_t *out,
                            uint8_t *weights, unsigned long long *stats4)
{
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y, cw = W0 / 2, ch = H0 / 2;
    // channel k of the pixel at the view's position (X, Y): 0 outside the frame
    const auto texel = [&](const uint8_t *img, int X, int Y, int k) {
        const int x = X - pad_x, y = Y - pad_y;
        return x < 0 || y < 0 || x >= width || y >= height ? 0 : (int)img[((size_t)y * width + x) * chans + k];
    };
    const uint8_t *frames[2] = {prev, next};
    const int16_t *grids[2] = {to_prev, to_next};
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx;
            const int ox = 2 * cx, oy = 2 * cy;
            int w[2] = {0, 0}, px[2] = {0, 0}, py[2] = {0, 0};
            for (int k = 0; k < 2; ++k) {
                if (!frames[k]) continue;
                px[k] = ox + grids[k][2 * c];
                py[k] = oy + grids[k][2 * c + 1];
                if (px[k] < 0 || py[k] < 0 || px[k] > W0 - 2 || py[k] > H0 - 2) continue;
                int cost = 0;
                for (int chn = 0; chn < chans; ++chn) {
                    int cc = 0;
                    for (int i = 0; i < 2; ++i)
                        for (int j = 0; j < 2; ++j)
                            cc += abs(texel(cur, ox + j, oy + i, chn) - texel(frames[k], px[k] + j, py[k] + i, chn));
                    if (cc > cost) cost = cc;
                }
                if (cost < thr) w[k] = 8 * (thr - cost) / thr;
            }
            const int S = 8 + w[0] + w[1];
            unsigned diff = 0;
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const int x = ox + j - pad_x, y = oy + i - pad_y;
                    const bool inside = x >= 0 && y >= 0 && x < width && y < height;
                    for (int chn = 0; chn < chans; ++chn) {
                        const int cpx = texel(cur, ox + j, oy + i, chn);
                        int acc = 8 * cpx + S / 2;
                        for (int k = 0; k < 2; ++k)
                            if (w[k]) acc += w[k] * texel(frames[k], px[k] + j, py[k] + i, chn);
                        const int v = acc / S;
                        if (out && inside) out[((size_t)y * width + x) * chans + chn] = (uint8_t)v;
                        diff += (unsigned)abs(v - cpx);
                    }
                }
            if (weights) weights[c] = (uint8_t)(w[0] | w[1] << 4);
            if (win.contains(cx, cy)) { s[0] += w[0] > 0; s[1] += w[1] > 0; s[2] += (unsigned)(w[0] + w[1]); s[3] += diff; }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
}

}  // namespace bbme

// ---------------------------------------------------------------------------------------
// C-ABI, host-only entry points
// ---------------------------------------------------------------------------------------
extern "C" {

const char *bbme_version(void) { return "bbme 0.1 (gfx950)"; }
const char *bbme_last_error(void) { return bbme::g_last_error.c_str(); }

int bbme_plan_padding(int width, int height, const bbme_params *params,
                      int *padded_width, int *padded_height, int *pad_x, int *pad_y)
{
    if (!params) return bbme::fail(BBME_ERR_INVALID, "params is null");
    if (int rc = bbme::validate_params(*params)) return rc;
    bbme::Geometry g;
    if (int rc = bbme::plan_padding(width, height, *params, g)) return rc;
    if (padded_width) *padded_width = g.padded_width;
    if (padded_height) *padded_height = g.padded_height;
    if (pad_x) *pad_x = g.pad_x;
    if (pad_y) *pad_y = g.pad_y;
    return BBME_OK;
}

int bbme_pad_zero_host(const uint8_t *src, int width, int height, int pitch, int pad_x, int pad_y, uint8_t *dst)
{
    if (!src || !dst || width <= 0 || height <= 0 || pitch < width || pad_x < 0 || pad_y < 0)
        return bbme::fail(BBME_ERR_INVALID, "bbme_pad_zero_host: bad arguments");
    bbme::pad_zero(src, width, height, pitch, pad_x, pad_y, dst);
    return BBME_OK;
}

int bbme_pyr_down_host(const uint8_t *src, int sw, int sh, uint8_t *dst)
{
    if (!src || !dst || sw < 2 || sh < 2) return bbme::fail(BBME_ERR_INVALID, "bbme_pyr_down_host: bad arguments");
    bbme::pyr_down(src, sw, sh, dst);
    return BBME_OK;
}

int bbme_resize_x4_host(const uint8_t *src, int sw, int sh, uint8_t *dst)
{
    if (!src || !dst || sw < 1 || sh < 1) return bbme::fail(BBME_ERR_INVALID, "bbme_resize_x4_host: bad arguments");
    bbme::resize_x4(src, sw, sh, dst);
    return BBME_OK;
}

int bbme_flo_read(const char *filename, int *width, int *height, float **data)
{
    if (!width || !height || !data) return bbme::fail(BBME_ERR_INVALID, "bbme_flo_read: null output");
    return bbme::flo_read(filename, width, height, data);
}

int bbme_flo_write(const char *filename, int width, int height, const float *data)
{
    return bbme::flo_write(filename, width, height, data);
}

int bbme_calculate_mse(const float *gtruth, const float *flow, int width, int height, double *out)
{
    if (!gtruth || !flow || !out || width < 1 || height < 1)
        return bbme::fail(BBME_ERR_INVALID, "bbme_calculate_mse: bad arguments");
    *out = bbme::calculate_mse(gtruth, flow, width, height);
    return BBME_OK;
}

int bbme_motion_to_color(const float *flow, int width, int height, float maxmotion, uint8_t *bgr, float *range)
{
    if (!flow || !bgr || width < 1 || height < 1)
        return bbme::fail(BBME_ERR_INVALID, "bbme_motion_to_color: bad arguments");
    bbme::motion_to_color(flow, width, height, maxmotion, bgr, range);
    return BBME_OK;
}

int bbme_ppm_write_bgr(const char *filename, int width, int height, const uint8_t *bgr)
{
    if (!filename || !bgr || width < 1 || height < 1)
        return bbme::fail(BBME_ERR_INVALID, "bbme_ppm_write_bgr: bad arguments");
    return bbme::ppm_write_bgr(filename, width, height, bgr);
}

int bbme_pgm_write(const char *filename, int width, int height, int pitch, const uint8_t *gray)
{
    if (!filename || !gray || width < 1 || height < 1 || pitch < width)
        return bbme::fail(BBME_ERR_INVALID, "bbme_pgm_write: bad arguments");
    FILE *f = fopen(filename, "wb");
    if (!f) return bbme::fail(BBME_ERR_IO, "pgm_write: could not open %s", filename);
    bool ok = fprintf(f, "P5\n%d %d\n255\n", width, height) > 0;
    for (int y = 0; y < height && ok; ++y) ok = fwrite(gray + (size_t)y * pitch, 1, (size_t)width, f) == (size_t)width;
    if (fclose(f) != 0) ok = false;
    return ok ? BBME_OK : bbme::fail(BBME_ERR_IO, "pgm_write: problem writing %s", filename);
}

int bbme_motion_compensate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *grid,
                                int grid_block, int block, int fill, const int *window, uint8_t *out, unsigned long long *stats4)
{
    if (!image2 || !grid || (!out && !stats4) || (stats4 && !image1))
        return bbme::fail(BBME_ERR_INVALID, "bbme_motion_compensate_host: null pointer");
    if (width < 1 || height < 1 || grid_block < 1 || block < 1 || (block & (block - 1)) || fill < 0 || fill > 255)
        return bbme::fail(BBME_ERR_INVALID, "bbme_motion_compensate_host: bad arguments (%dx%d, grid block %d, block %d, fill %d)",
                          width, height, grid_block, block, fill);
    bbme::CellWindow win;
    if (int rc = win.set(window, width, height, "bbme_motion_compensate_host", "plane")) return rc;
    bbme::motion_compensate(image1, image2, width, height, grid, grid_block, block, fill, win, out, stats4);
    return BBME_OK;
}

int bbme_cells_color_host(const int16_t *cells, int cells_w, int cells_h, int width, int height, int pad_x, int pad_y, int scale,
                          float maxmotion, uint8_t *bgr, float *range5)
{
    const char *what = "bbme_cells_color_host";
    if (!cells || (!bgr && !range5)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (scale < 1) return bbme::fail(BBME_ERR_INVALID, "%s: scale %d < 1", what, scale);
    if (cells_w < 1 || cells_h < 1 || width < 1 || height < 1 || pad_x < 0 || pad_y < 0 ||
        (long long)pad_x + width > 2LL * cells_w || (long long)pad_y + height > 2LL * cells_h)
        return bbme::fail(BBME_ERR_INVALID, "%s: the %dx%d frame at (%d, %d) is not inside the %dx%d cells", what, width, height,
                          pad_x, pad_y, cells_w, cells_h);
    bbme::cells_color(cells, cells_w, width, height, pad_x, pad_y, scale, maxmotion, bgr, range5);
    return BBME_OK;
}

int bbme_cells_consistency_host(const int16_t *a, const int16_t *b, int cells_w, int cells_h, int tol, const int *window,
                                uint8_t *mask, unsigned long long *stats4)
{
    if (!a || !b || (!mask && !stats4)) return bbme::fail(BBME_ERR_INVALID, "bbme_cells_consistency_host: null pointer");
    if (cells_w < 1 || cells_h < 1 || tol < 0)
        return bbme::fail(BBME_ERR_INVALID, "bbme_cells_consistency_host: bad arguments (%dx%d cells, tolerance %d)", cells_w, cells_h, tol);
    bbme::CellWindow win;
    if (int rc = win.set(window, cells_w, cells_h, "bbme_cells_consistency_host", "cells")) return rc;
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < cells_h; ++cy)
        for (int cx = 0; cx < cells_w; ++cx) {
            const size_t i = (size_t)cy * cells_w + cx;
            const int dx = a[2 * i], dy = a[2 * i + 1];
            const int tx = 2 * cx + dx, ty = 2 * cy + dy;
            int cls = BBME_FB_OUTSIDE;
            unsigned d = 0;
            if (tx >= 0 && ty >= 0 && tx < 2 * cells_w && ty < 2 * cells_h) {
                const size_t j = (size_t)(ty >> 1) * cells_w + (tx >> 1);
                d = (unsigned)(abs(dx + b[2 * j]) + abs(dy + b[2 * j + 1]));
                cls = d <= (unsigned)tol ? BBME_FB_CONSISTENT : BBME_FB_INCONSISTENT;
            }
            if (mask) mask[i] = (uint8_t)cls;
            if (win.contains(cx, cy)) { ++s[cls]; s[3] += d; }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
    return BBME_OK;
}

// The interpolation rule of include/bbme.h, cell by cell, in the header's own words (the mirror of k_interpolate).
int bbme_interpolate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *fwd,
                          const int16_t *bwd, int num, int den, const int *window, uint8_t *out, uint8_t *sel,
                          unsigned long long *stats4)
{
    if (!image1 || !image2 || !fwd || (!out && !sel && !stats4))
        return bbme::fail(BBME_ERR_INVALID, "bbme_interpolate_host: null pointer");
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "bbme_interpolate_host: %dx%d is not a plane of 2x2 cells", width, height);
    if (den < 2 || den > 256 || num < 1 || num >= den)
        return bbme::fail(BBME_ERR_INVALID, "bbme_interpolate_host: phase %d / %d (2 <= den <= 256, 0 < num < den)", num, den);
    const int cw = width / 2, ch = height / 2;
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, "bbme_interpolate_host", "cells")) return rc;
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx;
            const int ox = 2 * cx, oy = 2 * cy;
            int best = -1, best_cost = 0, b1x = 0, b1y = 0, b2x = 0, b2y = 0;
            for (int k = 0; k < 3; ++k) {
                if (k == 1 && !bwd) continue;
                const bbme::Hypothesis h = bbme::hypothesis(fwd, bwd, cw, cx, cy, k, num, den);
                if (h.p1x < 0 || h.p2x < 0 || h.p1x > width - 2 || h.p2x > width - 2 || h.p1y < 0 || h.p2y < 0 || h.p1y > height - 2 ||
                    h.p2y > height - 2)
                    continue;
                int cost = 0;
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j)
                        cost += abs((int)image1[(size_t)(h.p1y + i) * width + h.p1x + j] -
                                    (int)image2[(size_t)(h.p2y + i) * width + h.p2x + j]);
                if (best < 0 || cost < best_cost) { best = k; best_cost = cost; b1x = h.p1x; b1y = h.p1y; b2x = h.p2x; b2y = h.p2y; }
            }
            if (out)
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j)
                        out[(size_t)(oy + i) * width + ox + j] =
                            (uint8_t)(((den - num) * image1[(size_t)(b1y + i) * width + b1x + j] +
                                       num * image2[(size_t)(b2y + i) * width + b2x + j] + den / 2) / den);
            if (sel) sel[c] = (uint8_t)best;
            if (win.contains(cx, cy)) { ++s[best]; s[3] += (unsigned)best_cost; }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
    return BBME_OK;
}

// The temporal filter rule on grey planes: bbme::temporal_filter with one channel, the plane being the padded view.
int bbme_temporal_filter_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height,
                              const int16_t *to_prev, const int16_t *to_next, int thr, const int *window, uint8_t *out,
                              uint8_t *weights, unsigned long long *stats4)
{
    const char *what = "bbme_temporal_filter_host";
    if (!cur || (!out && !weights && !stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if ((prev == nullptr) != (to_prev == nullptr) || (next == nullptr) != (to_next == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its plane and its grid", what);
    if (!prev && !next) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    bbme::CellWindow win;
    if (int rc = win.set(window, width / 2, height / 2, what, "cells")) return rc;
    bbme::temporal_filter(prev, cur, next, 1, width, height, 0, 0, to_prev, to_next, thr, win, out, weights, stats4);
    return BBME_OK;
}

// The luma rule of include/bbme.h (the mirror of bgr_luma in bbme_kernels.hpp).
int bbme_bgr_to_gray_host(const uint8_t *bgr, int width, int height, int pitch, uint8_t *gray)
{
    if (!bgr || !gray) return bbme::fail(BBME_ERR_INVALID, "bbme_bgr_to_gray_host: null pointer");
    if (width < 1 || height < 1 || (long long)pitch < 3LL * width)
        return bbme::fail(BBME_ERR_INVALID, "bbme_bgr_to_gray_host: bad arguments (%dx%d, pitch %d)", width, height, pitch);
    for (int y = 0; y < height; ++y) {
        const uint8_t *p = bgr + (size_t)y * pitch;
        for (int x = 0; x < width; ++x, p += 3)
            gray[(size_t)y * width + x] = (uint8_t)((1868 * p[0] + 9617 * p[1] + 4899 * p[2] + 8192) >> 14);
    }
    return BBME_OK;
}

// The BGR interpolation rule of include/bbme.h: the selection of bbme_interpolate_host on the luma planes (its map tells which
// hypothesis; p1 and p2 follow from it), then the blend of the two colour frames pixel by pixel (the mirror of k_interpolate_bgr).
int bbme_interpolate_bgr_host(const uint8_t *luma1, const uint8_t *luma2, int padded_w, int padded_h, const uint8_t *bgr1,
                              const uint8_t *bgr2, int width, int height, int pad_x, int pad_y, const int16_t *fwd,
                              const int16_t *bwd, int num, int den, uint8_t *out)
{
    const char *what = "bbme_interpolate_bgr_host";
    if (!luma1 || !luma2 || !bgr1 || !bgr2 || !fwd || !out) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x != padded_w ||
        (long long)height + 2LL * pad_y != padded_h)
        return bbme::fail(BBME_ERR_INVALID, "%s: the %dx%d frame with padding (%d, %d) is not the %dx%d plane", what, width, height,
                          pad_x, pad_y, padded_w, padded_h);
    const int cw = padded_w / 2;
    std::vector<uint8_t> sel((size_t)cw * (padded_h / 2) + 1);
    if (int rc = bbme_interpolate_host(luma1, luma2, padded_w, padded_h, fwd, bwd, num, den, nullptr, nullptr, sel.data(), nullptr))
        return rc;                                            // odd planes and bad phases are refused there
    const auto texel = [&](const uint8_t *img, int x, int y, int c) {
        return x < 0 || y < 0 || x >= width || y >= height ? 0 : (int)img[((size_t)y * width + x) * 3 + c];
    };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const int X = x + pad_x, Y = y + pad_y, cx = X >> 1, cy = Y >> 1;
            const bbme::Hypothesis h = bbme::hypothesis(fwd, bwd, cw, cx, cy, sel[(size_t)cy * cw + cx], num, den);
            const int q1x = h.p1x + (X & 1) - pad_x, q1y = h.p1y + (Y & 1) - pad_y, q2x = q1x + h.vx, q2y = q1y + h.vy;
            for (int ch = 0; ch < 3; ++ch)
                out[((size_t)y * width + x) * 3 + ch] =
                    (uint8_t)(((den - num) * texel(bgr1, q1x, q1y, ch) + num * texel(bgr2, q2x, q2y, ch) + den / 2) / den);
        }
    return BBME_OK;
}

// The BGR temporal filter rule: bbme::temporal_filter with three channels, the frame inside its padded view.
int bbme_temporal_filter_bgr_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height, int pad_x,
                                  int pad_y, const int16_t *to_prev, const int16_t *to_next, int thr, const int *window, uint8_t *out,
                                  uint8_t *weights, unsigned long long *stats4)
{
    const char *what = "bbme_temporal_filter_bgr_host";
    if (!cur || (!out && !weights && !stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if ((prev == nullptr) != (to_prev == nullptr) || (next == nullptr) != (to_next == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its frame and its grid", what);
    if (!prev && !next) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x > INT32_MAX ||
        (long long)height + 2LL * pad_y > INT32_MAX)
        return bbme::fail(BBME_ERR_INVALID, "%s: bad frame %dx%d with padding (%d, %d)", what, width, height, pad_x, pad_y);
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y;
    if ((W0 & 1) || (H0 & 1)) return bbme::fail(BBME_ERR_INVALID, "%s: the padded view %dx%d is not a plane of 2x2 cells", what, W0, H0);
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    bbme::CellWindow win;
    if (int rc = win.set(window, W0 / 2, H0 / 2, what, "cells")) return rc;
    bbme::temporal_filter(prev, cur, next, 3, width, height, pad_x, pad_y, to_prev, to_next, thr, win, out, weights, stats4);
    return BBME_OK;
}

int bbme_subsample_div4(const float *flow_padded, int padded_width, int padded_height,
                        int pad_x, int pad_y, float *out, int out_width, int out_height)
{
    if (!flow_padded || !out) return bbme::fail(BBME_ERR_INVALID, "bbme_subsample_div4: null pointer");
    const int need_w = (padded_width - 2 * pad_x + 3) / 4, need_h = (padded_height - 2 * pad_y + 3) / 4;
    if (out_width < need_w || out_height < need_h)
        return bbme::fail(BBME_ERR_INVALID, "bbme_subsample_div4: output %dx%d smaller than %dx%d",
                          out_width, out_height, need_w, need_h);
    bbme::subsample_div4(flow_padded, padded_width, padded_height, pad_x, pad_y, out, out_width);
    return BBME_OK;
}

// The SUBPEL RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of k_subpel_refine).  A candidate's
// samples are taken the separable way the rule allows: the horizontal sums of the nine rows it touches, then the vertical sum
// with the single rounding.
int bbme_subpel_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *cells, const int *window,
                     int16_t *out_q4, unsigned long long *stats4)
{
    const char *what = "bbme_subpel_host";
    if (!image1 || !image2 || !cells || (!out_q4 && !stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (width > 8188 || height > 8188)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: %dx%d is beyond 8188 (quarter-pel vectors would not fit 16 bits)", what, width, height);
    const int cw = width / 2, ch = height / 2;
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, what, "cells")) return rc;
    const auto sat16 = [](int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); };
    static const int order[8][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {1, 0}, {-1, 1}, {0, 1}, {1, 1}};
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx;
            const int vx = cells[2 * c], vy = cells[2 * c + 1];
            const int ax = 2 * cx - 3, ay = 2 * cy - 3, bx = ax + vx, by = ay + vy;
            int qx = 0, qy = 0;
            if (ax >= 0 && ax + 8 <= width && ay >= 0 && ay + 8 <= height && bx >= 2 && bx + 10 <= width && by >= 2 && by + 10 <= height) {
                int ref[8][8], patch[10][10];                 // I1's window; I2 at b + (-1 .. 8, -1 .. 8)
                for (int i = 0; i < 8; ++i)
                    for (int j = 0; j < 8; ++j) ref[i][j] = image1[(size_t)(ay + i) * width + ax + j];
                for (int i = 0; i < 10; ++i)
                    for (int j = 0; j < 10; ++j) patch[i][j] = image2[(size_t)(by - 1 + i) * width + bx - 1 + j];
                const auto cost = [&](int cqx, int cqy) {
                    const int ix = cqx >> 2, iy = cqy >> 2, fx = cqx & 3, fy = cqy & 3;
                    int h[9][8];
                    for (int i = 0; i < 9; ++i)
                        for (int j = 0; j < 8; ++j)
                            h[i][j] = (4 - fx) * patch[1 + iy + i][1 + ix + j] + fx * patch[1 + iy + i][2 + ix + j];
                    int sum = 0;
                    for (int i = 0; i < 8; ++i)
                        for (int j = 0; j < 8; ++j) sum += abs(ref[i][j] - (((4 - fy) * h[i][j] + fy * h[i + 1][j] + 8) >> 4));
                    return sum;
                };
                const int cost0 = cost(0, 0);
                int best = cost0;
                for (int step = 2; step >= 1; --step) {
                    const int c0x = qx, c0y = qy;
                    for (const auto &d : order) {
                        const int k = cost(c0x + step * d[0], c0y + step * d[1]);
                        if (k < best) { best = k; qx = c0x + step * d[0]; qy = c0y + step * d[1]; }
                    }
                }
                if (win.contains(cx, cy)) {
                    ++s[0]; s[1] += qx != 0 || qy != 0; s[2] += (unsigned)cost0; s[3] += (unsigned)best;
                }
            }
            if (out_q4) { out_q4[2 * c] = sat16(4 * vx + qx); out_q4[2 * c + 1] = sat16(4 * vy + qy); }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
    return BBME_OK;
}

// The SUBPEL COMPENSATION RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of k_subpel_compensate).  A
// tap of weight 0 is not read: it may lie outside the plane.
int bbme_subpel_compensate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *q4, int fill,
                                const int *window, uint8_t *out, unsigned long long *stats4)
{
    const char *what = "bbme_subpel_compensate_host";
    if (!image2 || !q4 || (!out && !stats4) || (stats4 && !image1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (fill < 0 || fill > 255) return bbme::fail(BBME_ERR_INVALID, "%s: fill %d outside 0..255", what, fill);
    bbme::CellWindow win;
    if (int rc = win.set(window, width, height, what, "plane")) return rc;
    const int cw = width / 2, ch = height / 2;
    unsigned long long sse = 0, sad = 0, pixels = 0, skipped = 0;
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const int16_t *q = q4 + 2 * ((size_t)cy * cw + cx);
            const int ox = 2 * cx, oy = 2 * cy;
            const int ix = q[0] >> 2, iy = q[1] >> 2, fx = q[0] & 3, fy = q[1] & 3;
            const int sx = ox + ix, sy = oy + iy;
            const bool ok = 0 <= sx && sx + 2 + (fx != 0) <= width && 0 <= sy && sy + 2 + (fy != 0) <= height;
            for (int k = 0; k < 2; ++k)
                for (int j = 0; j < 2; ++j) {
                    int v = fill;
                    if (ok) {
                        const auto tap = [&](int weight, int dx, int dy) {
                            return weight ? weight * image2[(size_t)(sy + k + dy) * width + sx + j + dx] : 0;
                        };
                        v = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
                    }
                    const size_t at = (size_t)(oy + k) * width + ox + j;
                    if (out) out[at] = (uint8_t)v;
                    if (!stats4 || !win.contains(ox + j, oy + k)) continue;
                    if (!ok) { ++skipped; continue; }
                    const int d = v - image1[at];
                    sse += (unsigned long long)(d * d);
                    sad += (unsigned long long)(d < 0 ? -d : d);
                    ++pixels;
                }
        }
    if (stats4) { stats4[0] = sse; stats4[1] = sad; stats4[2] = pixels; stats4[3] = skipped; }
    return BBME_OK;
}

// ---- the GLOBAL MOTION RULE and the GLOBAL COMPENSATION RULE of include/bbme.h, in the header's own words (the mirrors of
// k_vector_histogram, k_global_moments and k_global_compensate) ---------------------------------------------------------------

// what the four calls on a grid check alike
static int gm_check_grid(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch, const char *what)
{
    if (!cells) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (cells_w < 1 || cells_h < 1) return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d cells", what, cells_w, cells_h);
    if (cells_w > 4094 || cells_h > 4094)
        return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: %dx%d cells are beyond a plane of 8188", what, cells_w, cells_h);
    if (exclude && exclude_pitch < cells_w)
        return bbme::fail(BBME_ERR_INVALID, "%s: exclusion mask pitch %d < %d cells per row", what, exclude_pitch, cells_w);
    return BBME_OK;
}

static int gm_check_fit(int kind, long long tol_q16, int iterations, const char *what)
{
    if (kind != BBME_GM_TRANSLATION && kind != BBME_GM_AFFINE) return bbme::fail(BBME_ERR_INVALID, "%s: kind = %d (0 or 1)", what, kind);
    if (tol_q16 < 0 || tol_q16 > (1LL << 40)) return bbme::fail(BBME_ERR_INVALID, "%s: tolerance %lld outside 0..2^40", what, tol_q16);
    if (iterations < 0 || iterations > 8) return bbme::fail(BBME_ERR_INVALID, "%s: %d iterations (0..8)", what, iterations);
    return BBME_OK;
}

int bbme_vector_histogram_host(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch,
                               const int *window, uint32_t *hist)
{
    const char *what = "bbme_vector_histogram_host";
    if (int rc = gm_check_grid(cells, cells_w, cells_h, exclude, exclude_pitch, what)) return rc;
    if (!hist) return bbme::fail(BBME_ERR_INVALID, "%s: null output", what);
    bbme::CellWindow win;
    if (int rc = win.set(window, cells_w, cells_h, what, "cells")) return rc;
    memset(hist, 0, 2 * BBME_GM_BINS * sizeof(uint32_t));
    for (int cy = win.y0; cy < win.y1; ++cy)
        for (int cx = win.x0; cx < win.x1; ++cx) {
            if (exclude && exclude[(size_t)cy * exclude_pitch + cx]) continue;
            const int16_t *v = cells + 2 * ((size_t)cy * cells_w + cx);
            for (int k = 0; k < 2; ++k) ++hist[k * BBME_GM_BINS + (v[k] < -1024 ? -1024 : v[k] > 1023 ? 1023 : v[k]) + 1024];
        }
    return BBME_OK;
}

int bbme_global_moments_host(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch,
                             const int32_t *model, long long tol_q16, const int *window, uint8_t *map, long long *words16)
{
    const char *what = "bbme_global_moments_host";
    if (int rc = gm_check_grid(cells, cells_w, cells_h, exclude, exclude_pitch, what)) return rc;
    if (!model || (!map && !words16)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = gm_check_fit(BBME_GM_TRANSLATION, tol_q16, 0, what)) return rc;
    bbme::CellWindow win;
    if (int rc = win.set(window, cells_w, cells_h, what, "cells")) return rc;
    unsigned long long s[16] = {};                            // two's-complement sums: no signed overflow whatever word 3 does
    for (int cy = 0; cy < cells_h; ++cy)
        for (int cx = 0; cx < cells_w; ++cx) {
            const size_t i = (size_t)cy * cells_w + cx;
            const long long X = 4LL * cx + 2 - 2LL * cells_w, Y = 4LL * cy + 2 - 2LL * cells_h, dx = cells[2 * i], dy = cells[2 * i + 1];
            int cls = BBME_GM_EXCLUDED;
            long long r = 0;
            if (!exclude || !exclude[(size_t)cy * exclude_pitch + cx]) {
                const long long pu = model[0] + model[1] * X + model[2] * Y, pv = model[3] + model[4] * X + model[5] * Y;
                r = llabs(dx * 65536 - pu) + llabs(dy * 65536 - pv);
                cls = r <= tol_q16 ? BBME_GM_INLIER : BBME_GM_OUTLIER;
            }
            if (map) map[i] = (uint8_t)cls;
            if (!win.contains(cx, cy)) continue;
            ++s[cls];
            if (cls != BBME_GM_INLIER) continue;
            const long long t[13] = {r, X, Y, X * X, X * Y, Y * Y, dx, dy, X * dx, Y * dx, X * dy, Y * dy, dx * dx + dy * dy};
            for (int k = 0; k < 13; ++k) s[3 + k] += (unsigned long long)t[k];
        }
    if (words16) memcpy(words16, s, sizeof s);
    return BBME_OK;
}

// llrint(v * 65536), half to even (the default rounding mode), saturated to int32
static int32_t gm_q16(double v)
{
    const double q = v * 65536.0;
    if (!(q > -2147483648.0)) return INT32_MIN;               // NaN too
    if (q >= 2147483647.0) return INT32_MAX;
    return (int32_t)llrint(q);
}

#if defined(__clang__)
#define BBME_NO_FP_CONTRACT
#elif defined(__GNUC__)
#define BBME_NO_FP_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define BBME_NO_FP_CONTRACT
#endif

BBME_NO_FP_CONTRACT int bbme_global_motion_solve_host(const long long *w, int kind, int32_t *model)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const char *what = "bbme_global_motion_solve_host";
    if (!w || !model) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = gm_check_fit(kind, 0, 0, what)) return rc;
    for (int k = 0; k < 6; ++k) model[k] = 0;
    if (w[0] <= 0) return BBME_OK;
    const double n = (double)w[0], sx = (double)w[4], sy = (double)w[5], su = (double)w[9], sv = (double)w[10];
    const double xm = sx / n, ym = sy / n, um = su / n, vm = sv / n;
    model[0] = gm_q16(um);
    model[3] = gm_q16(vm);
    if (kind != BBME_GM_AFFINE || w[0] < 3) return BBME_OK;
    const double Sxx = (double)w[6] - sx * xm, Sxy = (double)w[7] - sx * ym, Syy = (double)w[8] - sy * ym;
    const double D = Sxx * Syy - Sxy * Sxy;
    if (!(Sxx > 0.0 && Syy > 0.0 && D > Sxx * Syy / 1048576.0)) return BBME_OK;
    const double Sxu = (double)w[11] - sx * um, Syu = (double)w[12] - sy * um, Sxv = (double)w[13] - sx * vm, Syv = (double)w[14] - sy * vm;
    const double a1 = (Sxu * Syy - Syu * Sxy) / D, a2 = (Syu * Sxx - Sxu * Sxy) / D, a0 = um - a1 * xm - a2 * ym;
    const double b1 = (Sxv * Syy - Syv * Sxy) / D, b2 = (Syv * Sxx - Sxv * Sxy) / D, b0 = vm - b1 * xm - b2 * ym;
    model[0] = gm_q16(a0); model[1] = gm_q16(a1); model[2] = gm_q16(a2);
    model[3] = gm_q16(b0); model[4] = gm_q16(b1); model[5] = gm_q16(b2);
    return BBME_OK;
}

int bbme_global_motion_host(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch, int kind,
                            long long tol_q16, int iterations, const int *window, int32_t *model, long long *words16, uint8_t *map)
{
    const char *what = "bbme_global_motion_host";
    if (int rc = gm_check_grid(cells, cells_w, cells_h, exclude, exclude_pitch, what)) return rc;
    if (!model) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (int rc = gm_check_fit(kind, tol_q16, iterations, what)) return rc;
    std::vector<uint32_t> hist(2 * BBME_GM_BINS);
    if (int rc = bbme_vector_histogram_host(cells, cells_w, cells_h, exclude, exclude_pitch, window, hist.data())) return rc;
    unsigned long long n = 0;
    for (int b = 0; b < BBME_GM_BINS; ++b) n += hist[b];
    for (int k = 0; k < 6; ++k) model[k] = 0;
    long long w[16];
    if (n) {
        model[0] = bbme::global_median(hist.data(), n) * 65536;
        model[3] = bbme::global_median(hist.data() + BBME_GM_BINS, n) * 65536;
        for (int it = 0; it < iterations; ++it) {
            if (int rc = bbme_global_moments_host(cells, cells_w, cells_h, exclude, exclude_pitch, model, tol_q16, window, nullptr, w)) return rc;
            if (w[0] == 0) break;
            if (int rc = bbme_global_motion_solve_host(w, kind, model)) return rc;
        }
    }
    if (!map && !words16) return BBME_OK;
    return bbme_global_moments_host(cells, cells_w, cells_h, exclude, exclude_pitch, model, tol_q16, window, map, words16);
}

int bbme_global_compensate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int32_t *model, int unit,
                                int fill, const int *window, uint8_t *out, unsigned long long *stats4)
{
    const char *what = "bbme_global_compensate_host";
    if (!image2 || !model || (!out && !stats4) || (stats4 && !image1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (width > 8188 || height > 8188) return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: %dx%d is beyond 8188", what, width, height);
    if (unit != 1 && unit != 4) return bbme::fail(BBME_ERR_INVALID, "%s: unit %d (1 or 4)", what, unit);
    if (fill < 0 || fill > 255) return bbme::fail(BBME_ERR_INVALID, "%s: fill %d outside 0..255", what, fill);
    bbme::CellWindow win;
    if (int rc = win.set(window, width, height, what, "plane")) return rc;
    const long long mul = 4 / unit;
    unsigned long long sse = 0, sad = 0, pixels = 0, skipped = 0;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const long long X = 2LL * x + 1 - width, Y = 2LL * y + 1 - height;
            const long long pu = model[0] + model[1] * X + model[2] * Y, pv = model[3] + model[4] * X + model[5] * Y;
            const long long qx = (pu * mul + 32768) >> 16, qy = (pv * mul + 32768) >> 16;
            const int fx = (int)(qx & 3), fy = (int)(qy & 3);
            const long long sx = x + (qx >> 2), sy = y + (qy >> 2);
            const bool ok = 0 <= sx && sx + 1 + (fx != 0) <= width && 0 <= sy && sy + 1 + (fy != 0) <= height;
            int v = fill;
            if (ok) {
                const auto tap = [&](int weight, int dx, int dy) {
                    return weight ? weight * image2[(size_t)(sy + dy) * width + (size_t)(sx + dx)] : 0;
                };
                v = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
            }
            const size_t at = (size_t)y * width + x;
            if (out) out[at] = (uint8_t)v;
            if (!stats4 || !win.contains(x, y)) continue;
            if (!ok) { ++skipped; continue; }
            const int d = v - image1[at];
            sse += (unsigned long long)(d * d);
            sad += (unsigned long long)(d < 0 ? -d : d);
            ++pixels;
        }
    if (stats4) { stats4[0] = sse; stats4[1] = sad; stats4[2] = pixels; stats4[3] = skipped; }
    return BBME_OK;
}

// The BGR GLOBAL COMPENSATION RULE of include/bbme.h in the header's own words (the mirror of k_global_compensate_bgr): the grey
// rule on the zero-padded view of a colour frame, in frame coordinates.  A tap outside the frame is the padding's 0 and is not
// read; neither is a tap of weight 0.
int bbme_global_compensate_bgr_host(const uint8_t *bgr1, const uint8_t *bgr2, int width, int height, int bgr_pitch, int pad_x, int pad_y,
                                    const int32_t *model, int unit, int fill, const int *window, uint8_t *out, int out_pitch,
                                    unsigned long long *stats4)
{
    const char *what = "bbme_global_compensate_bgr_host";
    if (!bgr2 || !model || (!out && !stats4) || (stats4 && !bgr1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x > INT32_MAX ||
        (long long)height + 2LL * pad_y > INT32_MAX)
        return bbme::fail(BBME_ERR_INVALID, "%s: bad frame %dx%d with padding (%d, %d)", what, width, height, pad_x, pad_y);
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y;
    if ((W0 & 1) || (H0 & 1)) return bbme::fail(BBME_ERR_INVALID, "%s: the padded view %dx%d is not a plane of 2x2 cells", what, W0, H0);
    if (W0 > 8188 || H0 > 8188) return bbme::fail(BBME_ERR_UNSUPPORTED, "%s: the padded view %dx%d is beyond 8188", what, W0, H0);
    if (unit != 1 && unit != 4) return bbme::fail(BBME_ERR_INVALID, "%s: unit %d (1 or 4)", what, unit);
    if (fill < 0 || fill > 255) return bbme::fail(BBME_ERR_INVALID, "%s: fill %d outside 0..255", what, fill);
    if ((long long)bgr_pitch < 3LL * width) return bbme::fail(BBME_ERR_INVALID, "%s: colour pitch %d < 3 x frame width %d", what, bgr_pitch, width);
    if (out && (long long)out_pitch < 3LL * width)
        return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < 3 x frame width %d", what, out_pitch, width);
    bbme::CellWindow win;
    if (int rc = win.set(window, width, height, what, "frame")) return rc;
    const long long mul = 4 / unit;
    unsigned long long sse = 0, sad = 0, pixels = 0, skipped = 0;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const long long X = 2LL * x + 1 - width, Y = 2LL * y + 1 - height;      // = 2 (x + pad_x) + 1 - W0, 2 (y + pad_y) + 1 - H0
            const long long pu = model[0] + model[1] * X + model[2] * Y, pv = model[3] + model[4] * X + model[5] * Y;
            const long long qx = (pu * mul + 32768) >> 16, qy = (pv * mul + 32768) >> 16;
            const int fx = (int)(qx & 3), fy = (int)(qy & 3);
            const long long sx = x + (qx >> 2), sy = y + (qy >> 2);                  // frame coordinates: the padded plane's less the pads
            const bool ok = -pad_x <= sx && sx + 1 + (fx != 0) <= (long long)width + pad_x && -pad_y <= sy &&
                            sy + 1 + (fy != 0) <= (long long)height + pad_y;
            const size_t at = (size_t)y * bgr_pitch + (size_t)3 * x;
            for (int c = 0; c < 3; ++c) {
                int v = fill;
                if (ok) {
                    const auto tap = [&](int weight, int dx, int dy) {
                        const long long tx = sx + dx, ty = sy + dy;
                        if (!weight || tx < 0 || tx >= width || ty < 0 || ty >= height) return 0;
                        return weight * bgr2[(size_t)ty * bgr_pitch + (size_t)3 * tx + c];
                    };
                    v = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
                }
                if (out) out[(size_t)y * out_pitch + (size_t)3 * x + c] = (uint8_t)v;
                if (!stats4 || !ok || !win.contains(x, y)) continue;
                const int d = v - bgr1[at + c];
                sse += (unsigned long long)(d * d);
                sad += (unsigned long long)(d < 0 ? -d : d);
            }
            if (!stats4 || !win.contains(x, y)) continue;
            if (ok) ++pixels; else ++skipped;
        }
    if (stats4) { stats4[0] = sse; stats4[1] = sad; stats4[2] = pixels; stats4[3] = skipped; }
    return BBME_OK;
}

// The BGR COMPENSATION RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of k_compensate_bgr): the SUBPEL
// COMPENSATION RULE on the zero-padded view of a colour frame, in frame coordinates.  A tap outside the frame is the padding's 0
// and is not read; neither is a tap of weight 0.
int bbme_compensate_bgr_host(const uint8_t *bgr1, const uint8_t *bgr2, int width, int height, int bgr_pitch, int pad_x, int pad_y,
                             const int16_t *grid, int pitch_cells, int unit, int fill, const int *window, uint8_t *out, int out_pitch,
                             unsigned long long *stats4)
{
    const char *what = "bbme_compensate_bgr_host";
    if (!bgr2 || !grid || (!out && !stats4) || (stats4 && !bgr1)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x > INT32_MAX ||
        (long long)height + 2LL * pad_y > INT32_MAX)
        return bbme::fail(BBME_ERR_INVALID, "%s: bad frame %dx%d with padding (%d, %d)", what, width, height, pad_x, pad_y);
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y;
    if ((W0 & 1) || (H0 & 1)) return bbme::fail(BBME_ERR_INVALID, "%s: the padded view %dx%d is not a plane of 2x2 cells", what, W0, H0);
    if (unit != 1 && unit != 4) return bbme::fail(BBME_ERR_INVALID, "%s: unit %d (1 or 4)", what, unit);
    if (fill < 0 || fill > 255) return bbme::fail(BBME_ERR_INVALID, "%s: fill %d outside 0..255", what, fill);
    if ((long long)bgr_pitch < 3LL * width) return bbme::fail(BBME_ERR_INVALID, "%s: colour pitch %d < 3 x frame width %d", what, bgr_pitch, width);
    if (out && (long long)out_pitch < 3LL * width)
        return bbme::fail(BBME_ERR_INVALID, "%s: output pitch %d < 3 x frame width %d", what, out_pitch, width);
    const int cw = W0 / 2, ch = H0 / 2;
    if (pitch_cells < cw) return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, pitch_cells, cw);
    bbme::CellWindow win;
    if (int rc = win.set(window, width, height, what, "frame")) return rc;
    const int mul = 4 / unit;
    unsigned long long sse = 0, sad = 0, pixels = 0, skipped = 0;
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const int16_t *g = grid + 2 * ((size_t)cy * pitch_cells + cx);
            const int qx = mul * g[0], qy = mul * g[1];                              // 32 bits: 4 G need not fit int16
            const int fx = qx & 3, fy = qy & 3;
            const long long sx = 2LL * cx + (qx >> 2), sy = 2LL * cy + (qy >> 2);    // the padded plane's coordinates
            const bool ok = 0 <= sx && sx + 2 + (fx != 0) <= W0 && 0 <= sy && sy + 2 + (fy != 0) <= H0;
            for (int k = 0; k < 2; ++k)
                for (int j = 0; j < 2; ++j) {
                    const int x = 2 * cx + j - pad_x, y = 2 * cy + k - pad_y;        // the pixel in frame coordinates
                    if (x < 0 || x >= width || y < 0 || y >= height) continue;
                    const bool in = stats4 && win.contains(x, y);
                    for (int c = 0; c < 3; ++c) {
                        int v = fill;
                        if (ok) {
                            const auto tap = [&](int weight, int dx, int dy) {
                                const long long tx = sx + j + dx - pad_x, ty = sy + k + dy - pad_y;
                                if (!weight || tx < 0 || tx >= width || ty < 0 || ty >= height) return 0;
                                return weight * bgr2[(size_t)ty * bgr_pitch + (size_t)3 * tx + c];
                            };
                            v = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
                        }
                        if (out) out[(size_t)y * out_pitch + (size_t)3 * x + c] = (uint8_t)v;
                        if (!in || !ok) continue;
                        const int d = v - bgr1[(size_t)y * bgr_pitch + (size_t)3 * x + c];
                        sse += (unsigned long long)(d * d);
                        sad += (unsigned long long)(d < 0 ? -d : d);
                    }
                    if (!in) continue;
                    if (ok) ++pixels; else ++skipped;
                }
        }
    if (stats4) { stats4[0] = sse; stats4[1] = sad; stats4[2] = pixels; stats4[3] = skipped; }
    return BBME_OK;
}

// The SUBPEL INTERPOLATION RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of k_subpel_interpolate).
// A tap of weight 0 is not read: it may lie outside the plane.
int bbme_subpel_interpolate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *qf,
                                 const int16_t *qb, int num, int den, const int *window, uint8_t *out, uint8_t *sel,
                                 unsigned long long *stats4)
{
    const char *what = "bbme_subpel_interpolate_host";
    if (!image1 || !image2 || !qf || (!out && !sel && !stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (den < 2 || den > 256 || num < 1 || num >= den)
        return bbme::fail(BBME_ERR_INVALID, "%s: phase %d / %d (2 <= den <= 256, 0 < num < den)", what, num, den);
    const int cw = width / 2, ch = height / 2;
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, what, "cells")) return rc;
    const auto floor_div = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    // the four rounded samples of the cell at quarter-pel position (px, py) of `img`; false when a tap of non-zero weight leaves it
    const auto cell = [&](const uint8_t *img, int px, int py, int (&s)[4]) {
        const int ix = px >> 2, iy = py >> 2, fx = px & 3, fy = py & 3;
        if (ix < 0 || ix + 2 + (fx != 0) > width || iy < 0 || iy + 2 + (fy != 0) > height) return false;
        for (int r = 0; r < 2; ++r)
            for (int j = 0; j < 2; ++j) {
                const auto tap = [&](int weight, int dx, int dy) {
                    return weight ? weight * img[(size_t)(iy + r + dy) * width + ix + j + dx] : 0;
                };
                s[2 * r + j] = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
            }
        return true;
    };
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx;
            int best = -1, best_cost = 0, b1[4] = {0, 0, 0, 0}, b2[4] = {0, 0, 0, 0};
            for (int k = 0; k < 3; ++k) {
                if (k == 1 && !qb) continue;
                const int vx = k == 0 ? qf[2 * c] : k == 1 ? -(int)qb[2 * c] : 0, vy = k == 0 ? qf[2 * c + 1] : k == 1 ? -(int)qb[2 * c + 1] : 0;
                const int p1x = 8 * cx - floor_div(num * vx + den / 2, den), p1y = 8 * cy - floor_div(num * vy + den / 2, den);
                int s1[4], s2[4];
                if (!cell(image1, p1x, p1y, s1) || !cell(image2, p1x + vx, p1y + vy, s2)) continue;
                int cost = 0;
                for (int q = 0; q < 4; ++q) cost += abs(s1[q] - s2[q]);
                if (best < 0 || cost < best_cost) {
                    best = k; best_cost = cost;
                    memcpy(b1, s1, sizeof b1); memcpy(b2, s2, sizeof b2);
                }
            }
            if (out)
                for (int r = 0; r < 2; ++r)
                    for (int j = 0; j < 2; ++j)
                        out[(size_t)(2 * cy + r) * width + 2 * cx + j] = (uint8_t)(((den - num) * b1[2 * r + j] + num * b2[2 * r + j] + den / 2) / den);
            if (sel) sel[c] = (uint8_t)best;
            if (win.contains(cx, cy)) { ++s[best]; s[3] += (unsigned)best_cost; }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
    return BBME_OK;
}

// The SUBPEL TEMPORAL FILTER RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of
// k_subpel_temporal_filter).  A tap of weight 0 is not read: it may lie outside the plane.
int bbme_subpel_temporal_filter_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height,
                                     const int16_t *q_to_prev, const int16_t *q_to_next, int thr, const int *window, uint8_t *out,
                                     uint8_t *weights, unsigned long long *stats4)
{
    const char *what = "bbme_subpel_temporal_filter_host";
    if (!cur || (!out && !weights && !stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if ((prev == nullptr) != (q_to_prev == nullptr) || (next == nullptr) != (q_to_next == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its plane and its grid", what);
    if (!prev && !next) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    const int cw = width / 2, ch = height / 2;
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, what, "cells")) return rc;
    const uint8_t *frames[2] = {prev, next};
    const int16_t *grids[2] = {q_to_prev, q_to_next};
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx;
            const int ox = 2 * cx, oy = 2 * cy;
            int w[2] = {0, 0}, x[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};           // the weights; the rounded samples X'[j, k] at [2 k + j]
            for (int n = 0; n < 2; ++n) {
                if (!frames[n]) continue;
                const int qx = grids[n][2 * c], qy = grids[n][2 * c + 1];
                const int fx = qx & 3, fy = qy & 3, sx = ox + (qx >> 2), sy = oy + (qy >> 2);
                if (sx < 0 || sx + 2 + (fx != 0) > width || sy < 0 || sy + 2 + (fy != 0) > height) continue;
                int cost = 0;
                for (int k = 0; k < 2; ++k)
                    for (int j = 0; j < 2; ++j) {
                        const auto tap = [&](int weight, int dx, int dy) {
                            return weight ? weight * frames[n][(size_t)(sy + k + dy) * width + sx + j + dx] : 0;
                        };
                        x[n][2 * k + j] = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
                        cost += abs((int)cur[(size_t)(oy + k) * width + ox + j] - x[n][2 * k + j]);
                    }
                if (cost < thr) w[n] = 8 * (thr - cost) / thr;
            }
            const int S = 8 + w[0] + w[1];
            unsigned diff = 0;
            for (int k = 0; k < 2; ++k)
                for (int j = 0; j < 2; ++j) {
                    const size_t at = (size_t)(oy + k) * width + ox + j;
                    const int v = (8 * cur[at] + w[0] * x[0][2 * k + j] + w[1] * x[1][2 * k + j] + S / 2) / S;
                    if (out) out[at] = (uint8_t)v;
                    diff += (unsigned)abs(v - (int)cur[at]);
                }
            if (weights) weights[c] = (uint8_t)(w[0] | w[1] << 4);
            if (win.contains(cx, cy)) { s[0] += w[0] > 0; s[1] += w[1] > 0; s[2] += (unsigned)(w[0] + w[1]); s[3] += diff; }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
    return BBME_OK;
}

// What the BGR SUBPEL TEMPORAL FILTER RULE and the BGR WIDE TEMPORAL FILTER RULE say of ONE neighbour `frame` of the cell with origin
// (ox, oy) on the padded view of `cur` (both packed width x height B,G,R frames) and the quarter-pel vector (qx, qy): its weight,
// and channel k of the rounded sample X'[j, i] in x[2 i + j][k].  A tap of weight 0 or outside the frame is not read.
static int bgr_subpel_neighbour(const uint8_t *frame, const uint8_t *cur, int width, int height, int pad_x, int pad_y, int ox, int oy,
                                int qx, int qy, int thr, int (&x)[4][3])
{
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y;
    // channel k of the pixel at the padded position (X, Y) of a frame: 0 outside the frame
    const auto at = [&](const uint8_t *img, int X, int Y, int k) {
        const int px = X - pad_x, py = Y - pad_y;
        return px < 0 || py < 0 || px >= width || py >= height ? 0 : (int)img[((size_t)py * width + px) * 3 + k];
    };
    const int fx = qx & 3, fy = qy & 3, sx = ox + (qx >> 2), sy = oy + (qy >> 2);
    if (sx < 0 || sx + 2 + (fx != 0) > W0 || sy < 0 || sy + 2 + (fy != 0) > H0) return 0;
    int cost = 0;
    for (int k = 0; k < 3; ++k) {
        int cost_k = 0;
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
                const auto tap = [&](int weight, int dx, int dy) { return weight ? weight * at(frame, sx + j + dx, sy + i + dy, k) : 0; };
                x[2 * i + j][k] = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
                cost_k += abs(at(cur, ox + j, oy + i, k) - x[2 * i + j][k]);
            }
        cost = std::max(cost, cost_k);
    }
    return cost < thr ? 8 * (thr - cost) / thr : 0;
}

// The BGR SUBPEL TEMPORAL FILTER RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of
// k_subpel_temporal_filter_bgr).  A tap of weight 0 or outside the frame is not read.
int bbme_subpel_temporal_filter_bgr_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height, int pad_x,
                                         int pad_y, const int16_t *q_to_prev, const int16_t *q_to_next, int thr, const int *window,
                                         uint8_t *out, uint8_t *weights, unsigned long long *stats4)
{
    const char *what = "bbme_subpel_temporal_filter_bgr_host";
    if (!cur || (!out && !weights && !stats4)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if ((prev == nullptr) != (q_to_prev == nullptr) || (next == nullptr) != (q_to_next == nullptr))
        return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its frame and its grid", what);
    if (!prev && !next) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x > INT32_MAX ||
        (long long)height + 2LL * pad_y > INT32_MAX)
        return bbme::fail(BBME_ERR_INVALID, "%s: bad frame %dx%d with padding (%d, %d)", what, width, height, pad_x, pad_y);
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y;
    if ((W0 & 1) || (H0 & 1)) return bbme::fail(BBME_ERR_INVALID, "%s: the padded view %dx%d is not a plane of 2x2 cells", what, W0, H0);
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    const int cw = W0 / 2, ch = H0 / 2;
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, what, "cells")) return rc;
    const uint8_t *frames[2] = {prev, next};
    const int16_t *grids[2] = {q_to_prev, q_to_next};
    // channel k of the pixel at the padded position (X, Y) of a frame: 0 outside the frame
    const auto at = [&](const uint8_t *img, int X, int Y, int k) {
        const int x = X - pad_x, y = Y - pad_y;
        return x < 0 || y < 0 || x >= width || y >= height ? 0 : (int)img[((size_t)y * width + x) * 3 + k];
    };
    unsigned long long s[4] = {0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx;
            const int ox = 2 * cx, oy = 2 * cy;
            int w[2] = {0, 0}, x[2][4][3] = {};                // the weights; channel k of the rounded sample X'[j, i] at [2 i + j][k]
            for (int n = 0; n < 2; ++n)
                if (frames[n])
                    w[n] = bgr_subpel_neighbour(frames[n], cur, width, height, pad_x, pad_y, ox, oy, grids[n][2 * c], grids[n][2 * c + 1], thr, x[n]);
            const int S = 8 + w[0] + w[1];
            unsigned diff = 0;
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const int fxp = ox + j - pad_x, fyp = oy + i - pad_y;
                    const bool inside = fxp >= 0 && fyp >= 0 && fxp < width && fyp < height;
                    for (int k = 0; k < 3; ++k) {
                        const int cv = at(cur, ox + j, oy + i, k);
                        const int v = (8 * cv + w[0] * x[0][2 * i + j][k] + w[1] * x[1][2 * i + j][k] + S / 2) / S;
                        if (out && inside) out[((size_t)fyp * width + fxp) * 3 + k] = (uint8_t)v;
                        diff += (unsigned)abs(v - cv);
                    }
                }
            if (weights) weights[c] = (uint8_t)(w[0] | w[1] << 4);
            if (win.contains(cx, cy)) { s[0] += w[0] > 0; s[1] += w[1] > 0; s[2] += (unsigned)(w[0] + w[1]); s[3] += diff; }
        }
    if (stats4) memcpy(stats4, s, sizeof s);
    return BBME_OK;
}

// The CELL COMPOSITION RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of k_compose_cells).
int bbme_compose_host(const int16_t *a, int a_pitch_cells, const int16_t *b, int b_pitch_cells, int cells_w, int cells_h,
                      int unit_shift, const int *window, int16_t *out, int out_pitch_cells, unsigned long long *stats2)
{
    const char *what = "bbme_compose_host";
    if (!a || !b || (!out && !stats2)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (cells_w < 1 || cells_h < 1) return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d cells", what, cells_w, cells_h);
    if (a_pitch_cells < cells_w || b_pitch_cells < cells_w || (out && out_pitch_cells < cells_w))
        return bbme::fail(BBME_ERR_INVALID, "%s: a grid pitch < %d cells per row", what, cells_w);
    if (unit_shift != 0 && unit_shift != 2) return bbme::fail(BBME_ERR_INVALID, "%s: unit shift %d (0 or 2)", what, unit_shift);
    bbme::CellWindow win;
    if (int rc = win.set(window, cells_w, cells_h, what, "cells")) return rc;
    const int u = unit_shift;
    const auto sat16 = [](int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; };
    unsigned long long s[2] = {0, 0};
    for (int cy = 0; cy < cells_h; ++cy)
        for (int cx = 0; cx < cells_w; ++cx) {
            const size_t i = (size_t)cy * a_pitch_cells + cx;
            const int ax = a[2 * i], ay = a[2 * i + 1];
            const int tx = (2 * cx) * (1 << u) + ax, ty = (2 * cy) * (1 << u) + ay;
            // floor division by 2^(u + 1): the arithmetic shift of the rule, without shifting a negative number here
            const int d = 1 << (u + 1);
            const auto floor_div = [d](int v) { return v >= 0 ? v / d : -((-v + d - 1) / d); };
            const int px = floor_div(tx + (1 << u)), py = floor_div(ty + (1 << u));
            const int qx = std::min(std::max(px, 0), cells_w - 1), qy = std::min(std::max(py, 0), cells_h - 1);
            const size_t j = (size_t)qy * b_pitch_cells + qx;
            const int sx = ax + b[2 * j], sy = ay + b[2 * j + 1];
            const int rx = sat16(sx), ry = sat16(sy);
            if (out) {
                const size_t o = (size_t)cy * out_pitch_cells + cx;
                out[2 * o] = (int16_t)rx; out[2 * o + 1] = (int16_t)ry;
            }
            if (win.contains(cx, cy)) { s[0] += qx != px || qy != py; s[1] += rx != sx || ry != sy; }
        }
    if (stats2) memcpy(stats2, s, sizeof s);
    return BBME_OK;
}

// The WIDE TEMPORAL FILTER RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of
// k_wide_temporal_filter): bbme_subpel_temporal_filter_host's neighbour, up to four times.  A tap of weight 0 is not read.
int bbme_wide_temporal_filter_host(const uint8_t *const planes[4], const uint8_t *cur, int width, int height,
                                   const int16_t *const grids[4], int q4_pitch_cells, int thr, const int *window, uint8_t *out,
                                   uint16_t *weights, unsigned long long *stats6)
{
    const char *what = "bbme_wide_temporal_filter_host";
    if (!planes || !grids || !cur || (!out && !weights && !stats6)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    bool any = false;
    for (int n = 0; n < 4; ++n) {
        if ((planes[n] == nullptr) != (grids[n] == nullptr))
            return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its plane and its grid", what);
        any = any || planes[n];
    }
    if (!any) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (width < 2 || height < 2 || (width & 1) || (height & 1))
        return bbme::fail(BBME_ERR_INVALID, "%s: %dx%d is not a plane of 2x2 cells", what, width, height);
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    const int cw = width / 2, ch = height / 2;
    if (q4_pitch_cells < cw) return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, cw);
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, what, "cells")) return rc;
    unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx, g = (size_t)cy * q4_pitch_cells + cx;
            const int ox = 2 * cx, oy = 2 * cy;
            int w[4] = {0, 0, 0, 0}, x[4][4] = {};                               // the weights; the rounded samples X'[j, k] at [2 k + j]
            for (int n = 0; n < 4; ++n) {
                if (!planes[n]) continue;
                const int qx = grids[n][2 * g], qy = grids[n][2 * g + 1];
                const int fx = qx & 3, fy = qy & 3, sx = ox + (qx >> 2), sy = oy + (qy >> 2);
                if (sx < 0 || sx + 2 + (fx != 0) > width || sy < 0 || sy + 2 + (fy != 0) > height) continue;
                int cost = 0;
                for (int k = 0; k < 2; ++k)
                    for (int j = 0; j < 2; ++j) {
                        const auto tap = [&](int weight, int dx, int dy) {
                            return weight ? weight * planes[n][(size_t)(sy + k + dy) * width + sx + j + dx] : 0;
                        };
                        x[n][2 * k + j] = (tap((4 - fx) * (4 - fy), 0, 0) + tap(fx * (4 - fy), 1, 0) + tap((4 - fx) * fy, 0, 1) + tap(fx * fy, 1, 1) + 8) >> 4;
                        cost += abs((int)cur[(size_t)(oy + k) * width + ox + j] - x[n][2 * k + j]);
                    }
                if (cost < thr) w[n] = 8 * (thr - cost) / thr;
            }
            const int S = 8 + w[0] + w[1] + w[2] + w[3];
            unsigned diff = 0;
            for (int k = 0; k < 2; ++k)
                for (int j = 0; j < 2; ++j) {
                    const size_t at = (size_t)(oy + k) * width + ox + j;
                    int num = 8 * cur[at] + S / 2;
                    for (int n = 0; n < 4; ++n) num += w[n] * x[n][2 * k + j];
                    const int v = num / S;
                    if (out) out[at] = (uint8_t)v;
                    diff += (unsigned)abs(v - (int)cur[at]);
                }
            if (weights) weights[c] = (uint16_t)(w[0] | w[1] << 4 | w[2] << 8 | w[3] << 12);
            if (win.contains(cx, cy)) {
                for (int n = 0; n < 4; ++n) { s[n] += w[n] > 0; s[4] += (unsigned)w[n]; }
                s[5] += diff;
            }
        }
    if (stats6) memcpy(stats6, s, sizeof s);
    return BBME_OK;
}

// The BGR WIDE TEMPORAL FILTER RULE of include/bbme.h, cell by cell, in the header's own words (the mirror of
// k_wide_temporal_filter_bgr): bbme_subpel_temporal_filter_bgr_host's neighbour, up to four times, in bbme_wide_temporal_filter_host's
// blend, map and statistics.
int bbme_wide_temporal_filter_bgr_host(const uint8_t *const frames[4], const uint8_t *cur, int width, int height, int pad_x, int pad_y,
                                       const int16_t *const grids[4], int q4_pitch_cells, int thr, const int *window, uint8_t *out,
                                       uint16_t *weights, unsigned long long *stats6)
{
    const char *what = "bbme_wide_temporal_filter_bgr_host";
    if (!frames || !grids || !cur || (!out && !weights && !stats6)) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    bool any = false;
    for (int n = 0; n < 4; ++n) {
        if ((frames[n] == nullptr) != (grids[n] == nullptr))
            return bbme::fail(BBME_ERR_INVALID, "%s: a neighbour needs both its frame and its grid", what);
        any = any || frames[n];
    }
    if (!any) return bbme::fail(BBME_ERR_INVALID, "%s: no neighbour", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x > INT32_MAX ||
        (long long)height + 2LL * pad_y > INT32_MAX)
        return bbme::fail(BBME_ERR_INVALID, "%s: bad frame %dx%d with padding (%d, %d)", what, width, height, pad_x, pad_y);
    const int W0 = width + 2 * pad_x, H0 = height + 2 * pad_y;
    if ((W0 & 1) || (H0 & 1)) return bbme::fail(BBME_ERR_INVALID, "%s: the padded view %dx%d is not a plane of 2x2 cells", what, W0, H0);
    if (thr < 1 || thr > 1021) return bbme::fail(BBME_ERR_INVALID, "%s: strength %d outside 1..1021", what, thr);
    const int cw = W0 / 2, ch = H0 / 2;
    if (q4_pitch_cells < cw) return bbme::fail(BBME_ERR_INVALID, "%s: grid pitch %d < %d cells per row", what, q4_pitch_cells, cw);
    bbme::CellWindow win;
    if (int rc = win.set(window, cw, ch, what, "cells")) return rc;
    unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
    for (int cy = 0; cy < ch; ++cy)
        for (int cx = 0; cx < cw; ++cx) {
            const size_t c = (size_t)cy * cw + cx, g = (size_t)cy * q4_pitch_cells + cx;
            const int ox = 2 * cx, oy = 2 * cy;
            int w[4] = {0, 0, 0, 0}, x[4][4][3] = {};           // the weights; channel k of the rounded sample X'_n[j, i] at [n][2 i + j][k]
            for (int n = 0; n < 4; ++n)
                if (frames[n])
                    w[n] = bgr_subpel_neighbour(frames[n], cur, width, height, pad_x, pad_y, ox, oy, grids[n][2 * g], grids[n][2 * g + 1], thr, x[n]);
            const int S = 8 + w[0] + w[1] + w[2] + w[3];
            unsigned diff = 0;
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    const int fxp = ox + j - pad_x, fyp = oy + i - pad_y;
                    const bool inside = fxp >= 0 && fyp >= 0 && fxp < width && fyp < height;
                    for (int k = 0; k < 3; ++k) {
                        const int cv = inside ? (int)cur[((size_t)fyp * width + fxp) * 3 + k] : 0;
                        int num = 8 * cv + S / 2;
                        for (int n = 0; n < 4; ++n) num += w[n] * x[n][2 * i + j][k];
                        const int v = num / S;
                        if (out && inside) out[((size_t)fyp * width + fxp) * 3 + k] = (uint8_t)v;
                        diff += (unsigned)abs(v - cv);
                    }
                }
            if (weights) weights[c] = (uint16_t)(w[0] | w[1] << 4 | w[2] << 8 | w[3] << 12);
            if (win.contains(cx, cy)) {
                for (int n = 0; n < 4; ++n) { s[n] += w[n] > 0; s[4] += (unsigned)w[n]; }
                s[5] += diff;
            }
        }
    if (stats6) memcpy(stats6, s, sizeof s);
    return BBME_OK;
}

// The BGR SUBPEL INTERPOLATION RULE of include/bbme.h: the selection of bbme_subpel_interpolate_host on the luma planes (its map
// tells which hypothesis; P1 and P2 follow from it), then every pixel of the two colour frames sampled bilinearly at P1 and P2 and
// blended (the mirror of k_subpel_interpolate_bgr).  A tap of weight 0 or outside the frame is not read.
int bbme_subpel_interpolate_bgr_host(const uint8_t *luma1, const uint8_t *luma2, int padded_w, int padded_h, const uint8_t *bgr1,
                                     const uint8_t *bgr2, int width, int height, int pad_x, int pad_y, const int16_t *qf,
                                     const int16_t *qb, int num, int den, uint8_t *out)
{
    const char *what = "bbme_subpel_interpolate_bgr_host";
    if (!luma1 || !luma2 || !bgr1 || !bgr2 || !qf || !out) return bbme::fail(BBME_ERR_INVALID, "%s: null pointer", what);
    if (width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || (long long)width + 2LL * pad_x != padded_w ||
        (long long)height + 2LL * pad_y != padded_h)
        return bbme::fail(BBME_ERR_INVALID, "%s: the %dx%d frame with padding (%d, %d) is not the %dx%d plane", what, width, height,
                          pad_x, pad_y, padded_w, padded_h);
    const int cw = padded_w / 2;
    std::vector<uint8_t> sel((size_t)cw * (padded_h / 2) + 1);
    if (int rc = bbme_subpel_interpolate_host(luma1, luma2, padded_w, padded_h, qf, qb, num, den, nullptr, nullptr, sel.data(), nullptr))
        return rc;                                            // odd planes and bad phases are refused there
    const auto floor_div = [](int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    // channel ch of the frame's pixel sampled at integer position (tx, ty) with the fractions (fx, fy)
    const auto sample = [&](const uint8_t *img, int tx, int ty, int fx, int fy, int ch) {
        const auto tap = [&](int weight, int x, int y) {
            return !weight || x < 0 || y < 0 || x >= width || y >= height ? 0 : weight * (int)img[((size_t)y * width + x) * 3 + ch];
        };
        return (tap((4 - fx) * (4 - fy), tx, ty) + tap(fx * (4 - fy), tx + 1, ty) + tap((4 - fx) * fy, tx, ty + 1) +
                tap(fx * fy, tx + 1, ty + 1) + 8) >> 4;
    };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const int X = x + pad_x, Y = y + pad_y, cx = X >> 1, cy = Y >> 1;
            const size_t c = (size_t)cy * cw + cx;
            const int k = sel[c];
            const int vx = k == 0 ? qf[2 * c] : k == 1 ? -(int)qb[2 * c] : 0, vy = k == 0 ? qf[2 * c + 1] : k == 1 ? -(int)qb[2 * c + 1] : 0;
            const int p1x = 8 * cx - floor_div(num * vx + den / 2, den), p1y = 8 * cy - floor_div(num * vy + den / 2, den);
            const int p2x = p1x + vx, p2y = p1y + vy;
            const int t1x = (p1x >> 2) + (X & 1) - pad_x, t1y = (p1y >> 2) + (Y & 1) - pad_y;
            const int t2x = (p2x >> 2) + (X & 1) - pad_x, t2y = (p2y >> 2) + (Y & 1) - pad_y;
            for (int ch = 0; ch < 3; ++ch)
                out[((size_t)y * width + x) * 3 + ch] =
                    (uint8_t)(((den - num) * sample(bgr1, t1x, t1y, p1x & 3, p1y & 3, ch) +
                               num * sample(bgr2, t2x, t2y, p2x & 3, p2y & 3, ch) + den / 2) / den);
        }
    return BBME_OK;
}

int bbme_spiral_host(int search_size, int block_size, int16_t *dx, int16_t *dy, int capacity, int *count)
{
    if (!count) return bbme::fail(BBME_ERR_INVALID, "bbme_spiral_host: null count");
    const bbme::SpiralTable t = bbme::build_spiral(search_size, block_size);
    *count = (int)t.dx.size();
    if (dx && dy)
        for (int i = 0; i < *count && i < capacity; ++i) { dx[i] = t.dx[i]; dy[i] = t.dy[i]; }
    return BBME_OK;
}

int bbme_search_plan_host_waves(int range, int block_size, int waves, uint32_t *rounds, int rounds_capacity, int *nrounds,
                                uint32_t *tasks, int *groups, int *pitch_dw)
{
    if (!nrounds || range < 0 || range > 63 || (block_size != 8 && block_size != 16 && block_size != 32) || waves < 1 || waves > 2)
        return bbme::fail(BBME_ERR_INVALID, "bbme_search_plan_host: bad arguments");
    const int lanes = 64 * waves;
    const bbme::SearchPlan p = bbme::plan_search(range, block_size, waves == 2 || block_size == 32 ? 8 : 16, lanes,
                                                 getenv("BBME_LOOSE_PLAN") != nullptr);
    *nrounds = (int)p.rounds.size();
    if (groups) *groups = p.groups;
    if (pitch_dw) *pitch_dw = p.pitch_dw;
    for (int i = 0; i < *nrounds && i < rounds_capacity; ++i) {
        if (rounds) rounds[i] = p.rounds[i];
        if (tasks) memcpy(tasks + (size_t)i * lanes, p.tasks.data() + (size_t)i * lanes, lanes * sizeof(uint32_t));
    }
    return BBME_OK;
}

int bbme_search_plan_host(int range, int block_size, uint32_t *rounds, int rounds_capacity, int *nrounds,
                          uint32_t *tasks, int *groups, int *pitch_dw)
{
    return bbme_search_plan_host_waves(range, block_size, 1, rounds, rounds_capacity, nrounds, tasks, groups, pitch_dw);
}

void bbme_free(void *p) { free(p); }

// ---- asynchronous .flo writer: Flow::WriteFlowFile (rw_flow.cpp:139-200) on a worker thread ----
// The caller hands over a window of a (pinned) host buffer -- typically the padded field bbme_get_flow_host filled,
// with the padding stripped as main_class.cpp:63-70 does -- and goes on with the next pair; the worker writes the
// same bytes WriteFlowFile would ("PIEH", width, height, rows of interleaved u, v).  The buffer must stay untouched
// until bbme_flo_writer_wait returns.
struct bbme_flo_writer {
    struct Job {
        std::string name; int width, height; const float *data; size_t pitch_floats;
        const int16_t *cells; int cell_pitch, pad_x, pad_y;          // cells != nullptr: expand the 2x2-cell grid while writing
        unsigned long long ticket;
    };
    std::mutex mu;
    std::condition_variable cv_job, cv_idle;
    std::deque<Job> jobs;
    bool stop = false;
    int status = BBME_OK;
    std::string error;
    // tickets: job n is the n-th submitted (from 1); `finished` = every job up to it is on disk, `late` = finished jobs beyond
    // a gap (a pool of workers finishes files out of order)
    unsigned long long submitted = 0, finished = 0;
    std::set<unsigned long long> late;
    std::vector<std::thread> workers;
};

// copy_to_all_pixels (motion_framework.cpp:815-826) + the padding strip of main_class.cpp:63-70 + WriteFlowFile's rows, fused:
// pixel (x, y) of the file is the (dx, dy) of cell ((y + pad_y) / 2, (x + pad_x) / 2) as two floats.  The file is cut into bands
// of rows; a few threads expand bands into private buffers and pwrite them at their offsets (one thread fills ~5 GB/s, the
// 66 MB of a 4K field want more).
static bool flo_write_cells(const bbme_flo_writer::Job &job)
{
    const int fd = open(job.name.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return false;
    const size_t row_bytes = (size_t)job.width * 8;
    struct { char tag[4]; int32_t w, h; } head;
    memcpy(head.tag, bbme::kTagString, 4);
    head.w = job.width; head.h = job.height;
    // (measured on the GPU box's host, 66 MB per 4K field: 10 ms to tmpfs, 6 ms to the page cache, whatever the number of
    // threads -- the kernel's write path is the bound; mapping the file and expanding into the mapping was slower: 14-30 ms)
    std::atomic<bool> ok(pwrite(fd, &head, 12, 0) == 12);
    const int band = std::max(2, (int)((1u << 20) / row_bytes) & ~1);             // ~1 MB of output per band
    const int nbands = (job.height + band - 1) / band;
    int nthreads = 2;
    if (const char *e = getenv("BBME_WRITER_THREADS")) nthreads = atoi(e);
    nthreads = std::max(1, std::min(nthreads, std::min(nbands, 64)));
    std::atomic<int> next(0);
    auto work = [&]() {
        std::vector<float> buf((size_t)band * job.width * 2);
        for (int b = next.fetch_add(1); b < nbands && ok.load(); b = next.fetch_add(1)) {
            const int y0 = b * band, y1 = std::min(job.height, y0 + band);
            for (int y = y0; y < y1; ++y) {
                float *out = buf.data() + (size_t)(y - y0) * job.width * 2;
                const int py = y + job.pad_y;
                if (y > y0 && (py & 1)) {                                          // second row of a cell row: same values
                    memcpy(out, out - (size_t)job.width * 2, row_bytes);
                    continue;
                }
                const int16_t *crow = job.cells + (size_t)(py >> 1) * job.cell_pitch * 2;
                for (int x = 0; x < job.width; ++x) {
                    const int16_t *c = crow + (size_t)((x + job.pad_x) >> 1) * 2;
                    out[2 * x] = (float)c[0];
                    out[2 * x + 1] = (float)c[1];
                }
            }
            const size_t bytes = (size_t)(y1 - y0) * row_bytes;
            const char *src = reinterpret_cast<const char *>(buf.data());
            size_t done = 0;
            while (done < bytes) {
                const ssize_t n = pwrite(fd, src + done, bytes - done, (off_t)(12 + (size_t)y0 * row_bytes + done));
                if (n <= 0) { ok.store(false); break; }
                done += (size_t)n;
            }
        }
    };
    std::vector<std::thread> helpers;
    for (int i = 1; i < nthreads; ++i) helpers.emplace_back(work);
    work();
    for (auto &t : helpers) t.join();
    return (close(fd) == 0) && ok.load();
}

static void flo_writer_main(bbme_flo_writer *w)
{
    std::unique_lock<std::mutex> lk(w->mu);
    for (;;) {
        w->cv_job.wait(lk, [&] { return w->stop || !w->jobs.empty(); });
        if (w->jobs.empty()) return;
        bbme_flo_writer::Job job = w->jobs.front();
        w->jobs.pop_front();
        lk.unlock();
        bool ok = false;
        if (job.cells) ok = flo_write_cells(job);
        else if (FILE *f = fopen(job.name.c_str(), "wb")) {
            ok = fwrite(bbme::kTagString, 1, 4, f) == 4 && fwrite(&job.width, 4, 1, f) == 1 && fwrite(&job.height, 4, 1, f) == 1;
            const size_t row = (size_t)job.width * 2;
            if (job.pitch_floats == row) ok = ok && fwrite(job.data, sizeof(float), row * job.height, f) == row * job.height;
            else
                for (int y = 0; ok && y < job.height; ++y)
                    ok = fwrite(job.data + (size_t)y * job.pitch_floats, sizeof(float), row, f) == row;
            ok = (fclose(f) == 0) && ok;
        }
        lk.lock();
        if (!ok && w->status == BBME_OK) { w->status = BBME_ERR_IO; w->error = "WriteFlowFile: problem writing " + job.name; }
        w->late.insert(job.ticket);
        while (!w->late.empty() && *w->late.begin() == w->finished + 1) { w->late.erase(w->late.begin()); ++w->finished; }
        w->cv_idle.notify_all();
    }
}

int bbme_flo_writer_create(bbme_flo_writer **out) { return bbme_flo_writer_create_pool(1, out); }

int bbme_flo_writer_create_pool(int workers, bbme_flo_writer **out)
{
    if (!out) return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_create: null output");
    if (workers < 1 || workers > 64) return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_create_pool: %d workers (1..64)", workers);
    bbme_flo_writer *w = new bbme_flo_writer();
    for (int i = 0; i < workers; ++i) w->workers.emplace_back(flo_writer_main, w);
    *out = w;
    return BBME_OK;
}

int bbme_flo_writer_submit(bbme_flo_writer *w, const char *filename, int width, int height, const float *data,
                           int pitch_pixels)
{
    if (!w || !data || width < 1 || height < 1 || pitch_pixels < width)
        return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_submit: bad arguments");
    if (!filename) return bbme::fail(BBME_ERR_IO, "WriteFlowFile: empty filename");
    const char *dot = strrchr(filename, '.');
    if (!dot) return bbme::fail(BBME_ERR_IO, "WriteFlowFile: extension required in filename");
    if (strcmp(dot, ".flo") != 0) return bbme::fail(BBME_ERR_IO, "WriteFlowFile: filename should have extension '.flo'");
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->jobs.push_back({filename, width, height, data, (size_t)pitch_pixels * 2, nullptr, 0, 0, 0, ++w->submitted});
    }
    w->cv_job.notify_one();
    return BBME_OK;
}

int bbme_flo_writer_submit_cells(bbme_flo_writer *w, const char *filename, int width, int height, const int16_t *cells,
                                 int cell_rows, int cell_cols, int pad_x, int pad_y)
{
    if (!w || !cells || width < 1 || height < 1 || pad_x < 0 || pad_y < 0 || cell_rows < 1 || cell_cols < 1)
        return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_submit_cells: bad arguments");
    if (width + pad_x > 2 * cell_cols || height + pad_y > 2 * cell_rows)
        return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_submit_cells: a %dx%d window at (%d, %d) does not fit %dx%d cells of 2x2",
                          width, height, pad_x, pad_y, cell_cols, cell_rows);
    if (!filename) return bbme::fail(BBME_ERR_IO, "WriteFlowFile: empty filename");
    const char *dot = strrchr(filename, '.');
    if (!dot) return bbme::fail(BBME_ERR_IO, "WriteFlowFile: extension required in filename");
    if (strcmp(dot, ".flo") != 0) return bbme::fail(BBME_ERR_IO, "WriteFlowFile: filename should have extension '.flo'");
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->jobs.push_back({filename, width, height, nullptr, 0, cells, cell_cols, pad_x, pad_y, ++w->submitted});
    }
    w->cv_job.notify_one();
    return BBME_OK;
}

int bbme_flo_writer_ticket(bbme_flo_writer *w, unsigned long long *ticket)
{
    if (!w || !ticket) return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_ticket: null argument");
    std::lock_guard<std::mutex> lk(w->mu);
    *ticket = w->submitted;
    return BBME_OK;
}

int bbme_flo_writer_wait(bbme_flo_writer *w) { return bbme_flo_writer_wait_ticket(w, ~0ull); }

int bbme_flo_writer_wait_ticket(bbme_flo_writer *w, unsigned long long ticket)
{
    if (!w) return bbme::fail(BBME_ERR_INVALID, "bbme_flo_writer_wait: null writer");
    std::unique_lock<std::mutex> lk(w->mu);
    w->cv_idle.wait(lk, [&] { return w->finished >= std::min(ticket, w->submitted); });
    if (w->status != BBME_OK) {
        const int st = w->status;
        const std::string msg = w->error;
        w->status = BBME_OK; w->error.clear();
        return bbme::fail(st, "%s", msg.c_str());
    }
    return BBME_OK;
}

int bbme_flo_writer_destroy(bbme_flo_writer *w)
{
    if (!w) return BBME_OK;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->stop = true;
    }
    w->cv_job.notify_all();
    for (std::thread &t : w->workers) t.join();      // they finish the queued files first
    delete w;
    return BBME_OK;
}

}  // extern "C"
