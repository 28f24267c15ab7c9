// oracle/cvshim/opencv2/core/core.hpp -- stand-in for the part of OpenCV's core that the reference calls.
// TEST INFRASTRUCTURE ONLY.  Written by this project from the call sites in the reference's motion_framework.cpp,
// parallel.h, pyramid_level.h and rw_flow.*; it contains no line of OpenCV and no line of the reference.  Its only
// purpose is to let oracle/Makefile compile the reference's own core, in place, into oracle/_ref/mf_ref, so that the
// search, the regulariser, the level driver and the padding plan (all plain C++ in the reference) run as written.
//
// What it must honour, and why:
//   * Mat assignment and copy are shallow, clone() is deep: PyramidLevel keeps the padded planes by assignment
//     (motion_framework.cpp:68-70) and the constructor clones before pyrDown (:83-84, :102-103).
//   * a Rect view aliases its parent, and copyTo into a view writes the parent: draw_MVimage (:902) and
//     copyMakeBorder below rely on it.
//   * at<T>(i, j) takes int: the reference passes float indices (:441-521), which convert on the call.
//   * norm(a, b, NORM_L1) of two 8-bit blocks is the exact integer sum, returned as double (:265, :315, :599).
//   * Vec arithmetic is element by element in T (float32 for Vec2f), nothing fused (:576, :836).
//   * at<T> and operator()(Rect) CHECK BOUNDS and abort with a message, as OpenCV's own assertions do in a debug
//     build.  That turns the reference's undefined reads (a grid with fewer than two blocks in a dimension,
//     regularize_MVs :452-522) into something a test can see.
//   * every Mat has MAT_SLACK spare bytes behind its last element: rw_flow.cpp:242 writes three whole pixels
//     where it means three bytes, up to six bytes past the image when one of the last two pixels is unknown.
//   * pyrDown exists only so that MF::MF runs.  It is this project's restatement of OpenCV's published 5 x 5
//     kernel with reflect-101 borders; it PROVES NOTHING about OpenCV, and ref_mf_driver.cpp overwrites every
//     level's planes with injected ones before any comparison.
#ifndef BBME_CVSHIM_CORE_HPP
#define BBME_CVSHIM_CORE_HPP

#include <algorithm>
#include <cmath>
#include <math.h>       // the C++ <math.h>: puts the float overloads of sqrt, atan2, fabs and abs into the global namespace, where the
                        // reference's compiler has them (rw_flow.cpp:218, :256-257, :325 call them unqualified on floats and
                        // mean float arithmetic; with the double functions alone CalculateMSE moves in its ninth digit)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

typedef unsigned char uchar;
using std::isnan;       // rw_flow.cpp:42 calls a global isnan (MSVC's <math.h> has one)

// element kinds: kind * 16 + channels (our own encoding; only the three names below are used by the reference)
#define CVSHIM_KIND_U8 1
#define CVSHIM_KIND_S32 2
#define CVSHIM_KIND_F32 3
#define CV_8UC1 (CVSHIM_KIND_U8 * 16 + 1)
#define CV_8UC3 (CVSHIM_KIND_U8 * 16 + 3)
#define CV_32SC4 (CVSHIM_KIND_S32 * 16 + 4)
#define CV_32FC2 (CVSHIM_KIND_F32 * 16 + 2)

namespace cv {

enum { BORDER_CONSTANT = 0 };
enum { NORM_L1 = 2 };
enum { MAT_SLACK = 16 };

inline void shim_fail(const char *what, int a, int b, int c, int d)
{
    fprintf(stderr, "cvshim: %s (%d, %d) outside %d x %d\n", what, a, b, c, d);
    fflush(stderr);
    abort();
}

template <typename T, int N> struct Vec {
    T val[N];
    Vec() { for (int i = 0; i < N; ++i) val[i] = T(0); }
    Vec(T v0) { for (int i = 0; i < N; ++i) val[i] = T(0); val[0] = v0; }     // first element v0, the rest zero
    Vec(T v0, T v1) { for (int i = 0; i < N; ++i) val[i] = T(0); val[0] = v0; val[1] = v1; }
    Vec(T v0, T v1, T v2) { for (int i = 0; i < N; ++i) val[i] = T(0); val[0] = v0; val[1] = v1; val[2] = v2; }
    Vec(T v0, T v1, T v2, T v3) { val[0] = v0; val[1] = v1; val[2] = v2; val[3] = v3; }
    T &operator[](int i) { return val[i]; }
    const T &operator[](int i) const { return val[i]; }
    Vec mul(const Vec &o) const { Vec r; for (int i = 0; i < N; ++i) r.val[i] = (T)(val[i] * o.val[i]); return r; }
    Vec operator+(const Vec &o) const { Vec r; for (int i = 0; i < N; ++i) r.val[i] = (T)(val[i] + o.val[i]); return r; }
    bool operator==(const Vec &o) const { for (int i = 0; i < N; ++i) if (val[i] != o.val[i]) return false; return true; }
};
typedef Vec<float, 2> Vec2f;
typedef Vec<float, 4> Vec4f;
typedef Vec<int, 4> Vec4i;
typedef Vec<uchar, 3> Vec3b;

struct Scalar {
    double val[4];
    Scalar(double a = 0, double b = 0, double c = 0, double d = 0) { val[0] = a; val[1] = b; val[2] = c; val[3] = d; }
};
struct Size {
    int width, height;
    Size(int w = 0, int h = 0) : width(w), height(h) {}
    bool operator==(const Size &o) const { return width == o.width && height == o.height; }
    bool operator!=(const Size &o) const { return !(*this == o); }
};
struct Rect { int x, y, width, height; Rect(int x_ = 0, int y_ = 0, int w = 0, int h = 0) : x(x_), y(y_), width(w), height(h) {} };
struct Point { int x, y; Point(int x_ = 0, int y_ = 0) : x(x_), y(y_) {} };
struct Range { int start, end; Range(int s = 0, int e = 0) : start(s), end(e) {} };

struct Mat {
    int rows, cols;
    int type_;
    size_t step;                                   // bytes from one row to the next (a view keeps its parent's)
    uchar *data;
    std::shared_ptr<std::vector<uchar> > buf;      // shared by every shallow copy and view

    static int channels_of(int t) { return t % 16; }
    static size_t elem_size_of(int t) { return (size_t)(t % 16) * (t / 16 == CVSHIM_KIND_U8 ? 1 : 4); }

    Mat() : rows(0), cols(0), type_(0), step(0), data(0) {}
    Mat(int r, int c, int t) { create(r, c, t); }
    Mat(int r, int c, int t, const Scalar &s) { create(r, c, t); fill(s); }
    void create(int r, int c, int t)
    {
        if (r < 0 || c < 0) shim_fail("Mat of negative size", r, c, 0, 0);
        rows = r; cols = c; type_ = t; step = elem_size_of(t) * (size_t)c;
        buf.reset(new std::vector<uchar>(step * (size_t)r + MAT_SLACK));
        data = buf->data();
    }
    void fill(const Scalar &s)
    {
        const int cn = channels_of(type_), kind = type_ / 16;
        for (int i = 0; i < rows; ++i)
            for (int j = 0; j < cols; ++j)
                for (int k = 0; k < cn; ++k) {
                    uchar *p = data + (size_t)i * step + (size_t)j * elem_size_of(type_);
                    if (kind == CVSHIM_KIND_F32) ((float *)p)[k] = (float)s.val[k];
                    else if (kind == CVSHIM_KIND_S32) ((int *)p)[k] = (int)s.val[k];
                    else p[k] = (uchar)s.val[k];
                }
    }
    static Mat zeros(int r, int c, int t) { return Mat(r, c, t, Scalar(0, 0, 0, 0)); }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return data == 0 || rows == 0 || cols == 0; }
    int type() const { return type_; }
    int channels() const { return channels_of(type_); }

    template <typename T> T &at(int i, int j)
    {
        if (i < 0 || j < 0 || i >= rows || j >= cols) shim_fail("Mat::at", i, j, rows, cols);
        if (sizeof(T) != elem_size_of(type_)) shim_fail("Mat::at element size", (int)sizeof(T), (int)elem_size_of(type_), rows, cols);
        return *(T *)(data + (size_t)i * step + (size_t)j * sizeof(T));
    }
    template <typename T> const T &at(int i, int j) const { return const_cast<Mat *>(this)->at<T>(i, j); }

    Mat operator()(const Rect &r) const
    {
        if (r.x < 0 || r.y < 0 || r.width < 0 || r.height < 0 || r.x + r.width > cols || r.y + r.height > rows) {
            fprintf(stderr, "cvshim: Mat(Rect) x %d y %d w %d h %d ", r.x, r.y, r.width, r.height);
            shim_fail("view", r.x + r.width, r.y + r.height, rows, cols);
        }
        Mat m(*this);
        m.rows = r.height; m.cols = r.width;
        m.data = data + (size_t)r.y * step + (size_t)r.x * elem_size_of(type_);
        return m;
    }
    Mat clone() const
    {
        Mat m(rows, cols, type_);
        for (int i = 0; i < rows; ++i) memcpy(m.data + (size_t)i * m.step, data + (size_t)i * step, m.step);
        return m;
    }
    // copyTo into a Mat of the same size and type (a view included) writes that Mat's memory; anything else is
    // allocated anew, as OpenCV's create() would
    void copyTo(Mat &dst) const
    {
        if (dst.rows != rows || dst.cols != cols || dst.type_ != type_ || dst.data == 0) dst.create(rows, cols, type_);
        for (int i = 0; i < rows; ++i) memcpy(dst.data + (size_t)i * dst.step, data + (size_t)i * step, elem_size_of(type_) * (size_t)cols);
    }
    void copyTo(const Mat &view) const { Mat d(view); copyTo(d); if (d.data != view.data) shim_fail("copyTo into a view of another size", rows, cols, view.rows, view.cols); }
};

// exact integer sum of absolute differences of two 8-bit single-channel blocks, as double
inline double norm(const Mat &a, const Mat &b, int /*NORM_L1*/)
{
    if (a.rows != b.rows || a.cols != b.cols || a.type_ != CV_8UC1 || b.type_ != CV_8UC1) shim_fail("norm of unlike blocks", a.rows, a.cols, b.rows, b.cols);
    long long total = 0;
    for (int i = 0; i < a.rows; ++i) {
        const uchar *p = a.data + (size_t)i * a.step, *q = b.data + (size_t)i * b.step;
        int s = 0;
        for (int j = 0; j < a.cols; ++j) s += std::abs((int)p[j] - (int)q[j]);
        total += s;
    }
    return (double)total;
}

inline void copyMakeBorder(const Mat &src, Mat &dst, int top, int bottom, int left, int right, int /*BORDER_CONSTANT*/, const Scalar &v)
{
    Mat out(src.rows + top + bottom, src.cols + left + right, src.type_, v);
    src.copyTo(out(Rect(left, top, src.cols, src.rows)));
    dst = out;
}

// NOT OpenCV and no evidence about it: see the head of this file
inline int shim_reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}
inline void pyrDown(const Mat &src, Mat &dst, const Size &sz)
{
    static const int k[5] = {1, 4, 6, 4, 1};
    Mat out(sz.height, sz.width, CV_8UC1);
    for (int y = 0; y < sz.height; ++y)
        for (int x = 0; x < sz.width; ++x) {
            int s = 0;
            for (int dy = -2; dy <= 2; ++dy) {
                const uchar *row = src.data + (size_t)shim_reflect101(2 * y + dy, src.rows) * src.step;
                for (int dx = -2; dx <= 2; ++dx) s += k[dy + 2] * k[dx + 2] * row[shim_reflect101(2 * x + dx, src.cols)];
            }
            out.data[(size_t)y * out.step + x] = (uchar)((s + 128) >> 8);
        }
    dst = out;
}

inline void line(Mat &, Point, Point, const Scalar &) {}        // draw_MVs (:882) is debugging output; never called

struct ParallelLoopBody {
    virtual ~ParallelLoopBody() {}
    virtual void operator()(const Range &r) const = 0;
};
// serial: the whole range in one call, in order
inline void parallel_for_(const Range &r, const ParallelLoopBody &body) { body(r); }

}  // namespace cv
#endif
