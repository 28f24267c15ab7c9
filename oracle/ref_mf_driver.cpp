// ref_mf_driver.cpp -- caller of the reference's OWN core: MF (motion_framework.cpp, parallel.h) and Flow (rw_flow.cpp).
// TEST INFRASTRUCTURE ONLY.  This file contains no reference code: it only calls the reference's functions, which
// oracle/Makefile compiles from the reference directory in place, against the stand-in headers of oracle/cvshim/,
// into oracle/_ref/mf_ref.  Used to pin the oracle (tests/test_reference_core_cpu.py) and, through recorded
// digests, the kernels (tests/test_gpu_reference.py).  MF's private members are reached by opening `private` around
// the reference's header (the standard headers are included first, so that only the reference's classes are affected).
//
// All arrays travel as raw little-endian binary files; int32 headers, uint8 planes, float32 (u, v) grids, row-major.
//
//   mf_ref plan <out.txt> L b[0..L) w0 w1 h0 h1
//       MF::MF alone (:4-111) on zero images of every size w0 <= w < w1, h0 <= h < h1, each in a child process with stdin
//       closed (the reference answers an impossible size with getchar(); exit(1), :21-26).  One line per size:
//       "w h status padded_width padded_height padding_x padding_y"; status is the child's exit status.
//   mf_ref stages [--raster | --parallel] <in> <out>
//       in : L W H inject, search[L], block[L], frame1, frame2 (H x W); if inject: per level plane1, plane2
//       out: padded_width padded_height padding_x padding_y has_whole; per level plane1, plane2 as used;
//            the loop of :115-206 driven call by call (copyMVs, calcLevelBM, regularize_MVs with lambda_multiplier 1 and 2,
//            divide_blocks): after calcLevelBM and after every regularize_MVs the grid of level_flow at that call's
//            block size; then the dense field after copy_to_all_pixels; then (has_whole) the dense field of a second,
//            untouched MF run through calcMotionBlockMatching() whole, so that the schedule itself is the reference's.
//       --raster  : calcLevelBM's loop (:229-243) restated here around find_min_block (:246-294, dead code in the
//                   reference: :235 is commented out); no whole run (the reference's schedule calls the spiral)
//       --parallel: calcLevelBM_Parallel (:221-224) through the stand-in's serial parallel_for_; no whole run
//   mf_ref sweeps <in> <out>
//       in : W H B b search nm, mult[nm], plane1, plane2, grid (H/b x W/b x 2 float32)
//       out: the grid after each regularize_MVs at block size b, lambda = (B / 2) * (B / b), one per multiplier
//   mf_ref search-from-coarse <in> <out>
//       in : W H, search[2], block[2], plane1_l0, plane2_l0, plane1_l1, plane2_l1, level-1 grid at 2 x 2 cells
//       out: level 0's grid at block[0] after copyMVs + calcLevelBM
//   mf_ref mc <in> <out>
//       in : W H b fill, plane2, grid (H/b x W/b x 2 float32);  out: draw_MVimage (:887-905) into an H x W image of `fill`
//   mf_ref color <in> <out>     in: W H, float32 maxmotion, flow;   out: Flow::MotionToColor's B,G,R bytes
//   mf_ref mse <in> <out>       in: W H, ground truth, flow;        out: Flow::CalculateMSE's double
//
// Exit status: 0 ok, 1 the reference's own exit, 2 usage / short input, 3 a size that needs padding where none is allowed;
// a bounds check of the stand-in aborts with its message on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <queue>
#include <string>
#include <vector>
#include <sys/wait.h>
#include <unistd.h>
#include <fcntl.h>
#include <opencv2/core/core.hpp>
#include <opencv2/highgui/highgui.hpp>

#define private public
#include "motion_framework.h"
#undef private
#include "rw_flow.h"

typedef cv::Mat Mat;

static FILE *g_in, *g_out;

static void need(bool ok, const char *what)
{
    if (!ok) { fprintf(stderr, "mf_ref: %s\n", what); exit(2); }
}
static void get(void *p, size_t n) { need(fread(p, 1, n, g_in) == n, "input file too short"); }
static void put(const void *p, size_t n) { need(fwrite(p, 1, n, g_out) == n, "cannot write the output"); }
static std::vector<int> get_ints(int n) { std::vector<int> v(n); if (n) get(v.data(), 4 * (size_t)n); return v; }
static void get_plane(Mat &m) { for (int i = 0; i < m.rows; ++i) get(m.data + (size_t)i * m.step, (size_t)m.cols); }
static void put_plane(const Mat &m) { for (int i = 0; i < m.rows; ++i) put(m.data + (size_t)i * m.step, (size_t)m.cols); }
static void put_grid(Mat &flow, int b)
{
    for (int i = 0; i < flow.rows; i += b)
        for (int j = 0; j < flow.cols; j += b) put(&flow.at<cv::Vec2f>(i, j), 8);
}
static void get_grid(Mat &flow, int b)
{
    for (int i = 0; i < flow.rows; i += b)
        for (int j = 0; j < flow.cols; j += b) get(&flow.at<cv::Vec2f>(i, j), 8);
}

// calcLevelBM with find_min_block in the place of find_min_block_spiral
static void raster_level_bm(MF &mf)
{
    PyramidLevel &lv = mf.level_data[mf.curr_level];
    for (int y = 0; y < lv.image1.rows; y += lv.block_size)
        for (int x = 0; x < lv.image1.cols; x += lv.block_size) {
            cv::Vec2f &mv = lv.level_flow.at<cv::Vec2f>(y, x);
            BlockPosition hit = mf.find_min_block(y, x, y + (int)mv[1], x + (int)mv[0]);
            mv = cv::Vec2f((float)hit.pos_x - x, (float)hit.pos_y - y);
        }
}

static int cmd_plan(int argc, char **argv)
{
    need(argc >= 4, "plan: arguments");
    int L = atoi(argv[3]);
    need(L > 0 && argc == 4 + L + 4, "plan: arguments");
    std::vector<int> block(L), search(L);
    for (int i = 0; i < L; ++i) { block[i] = atoi(argv[4 + i]); search[i] = block[i]; }
    int w0 = atoi(argv[4 + L]), w1 = atoi(argv[5 + L]), h0 = atoi(argv[6 + L]), h1 = atoi(argv[7 + L]);
    FILE *out = fopen(argv[2], "w");
    need(out != 0, "plan: cannot open the output");
    for (int w = w0; w < w1; ++w)
        for (int h = h0; h < h1; ++h) {
            int fd[2];
            need(pipe(fd) == 0, "pipe");
            fflush(0);
            pid_t pid = fork();
            need(pid >= 0, "fork");
            if (pid == 0) {
                close(fd[0]);
                int nul = open("/dev/null", O_RDWR);
                dup2(nul, 0); dup2(nul, 1);             // getchar() meets end of file; the reference's message is dropped
                Mat a = Mat::zeros(h, w, CV_8UC1), b = Mat::zeros(h, w, CV_8UC1);
                MF mf(a, b, search.data(), block.data(), L);
                int geo[4] = {mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y};
                if (write(fd[1], geo, sizeof geo) != (ssize_t)sizeof geo) _exit(99);
                _exit(0);
            }
            close(fd[1]);
            int geo[4] = {0, 0, 0, 0}, status = 0;
            ssize_t got = read(fd[0], geo, sizeof geo);
            close(fd[0]);
            waitpid(pid, &status, 0);
            int code = WIFEXITED(status) ? WEXITSTATUS(status) : 128 + WTERMSIG(status);
            if (code == 0 && got != (ssize_t)sizeof geo) code = 98;
            fprintf(out, "%d %d %d %d %d %d %d\n", w, h, code, geo[0], geo[1], geo[2], geo[3]);
        }
    fclose(out);
    return 0;
}

static int cmd_stages(int mode /* 0 spiral, 1 raster, 2 parallel */)
{
    std::vector<int> hdr = get_ints(4);
    const int L = hdr[0], W = hdr[1], H = hdr[2], inject = hdr[3];
    need(L > 0 && L < 16 && W > 0 && H > 0, "stages: header");
    std::vector<int> search = get_ints(L), block = get_ints(L);
    Mat f1(H, W, CV_8UC1), f2(H, W, CV_8UC1);
    get_plane(f1); get_plane(f2);
    MF a(f1, f2, search.data(), block.data(), L), whole(f1, f2, search.data(), block.data(), L);
    if (inject)
        for (int l = 0; l < L; ++l) {
            get_plane(a.level_data[l].image1); get_plane(a.level_data[l].image2);
            a.level_data[l].image1.copyTo(whole.level_data[l].image1);
            a.level_data[l].image2.copyTo(whole.level_data[l].image2);
        }
    int geo[5] = {a.padded_width, a.padded_height, a.padding_x, a.padding_y, mode == 0};
    put(geo, sizeof geo);
    for (int l = 0; l < L; ++l) { put_plane(a.level_data[l].image1); put_plane(a.level_data[l].image2); }
    for (int l = L - 1; l >= 0; --l) {
        PyramidLevel &lv = a.level_data[l];
        a.curr_level = l;
        if (l != L - 1) a.copyMVs();
        if (mode == 1) raster_level_bm(a);
        else if (mode == 2) a.calcLevelBM_Parallel();
        else a.calcLevelBM();
        put_grid(lv.level_flow, lv.block_size);
        const int B = lv.block_size;
        const float lambda = lv.lambda;
        while (lv.block_size > 1) {
            for (int m = 1; m <= 2; ++m) {
                a.lambda_multiplier = m;
                a.regularize_MVs();
                put_grid(lv.level_flow, lv.block_size);
            }
            a.divide_blocks();
            lv.block_size >>= 1;
            lv.lambda = lv.lambda * 2;
        }
        lv.block_size = B;
        lv.lambda = lambda;
    }
    a.level_data[0].block_size = 2;
    a.copy_to_all_pixels();
    put_grid(a.level_data[0].level_flow, 1);
    if (mode == 0) {
        Mat flow = whole.calcMotionBlockMatching();
        put_grid(flow, 1);
    }
    return 0;
}

static int cmd_sweeps()
{
    std::vector<int> h = get_ints(6);
    int W = h[0], H = h[1], B = h[2], b = h[3], search = h[4], nm = h[5];
    std::vector<int> mults = get_ints(nm);
    Mat f1(H, W, CV_8UC1), f2(H, W, CV_8UC1);
    get_plane(f1); get_plane(f2);
    MF a(f1, f2, &search, &B, 1);
    if (a.padding_x || a.padding_y || a.padded_width != W || a.padded_height != H) return 3;
    a.curr_level = 0;
    PyramidLevel &lv = a.level_data[0];
    get_grid(lv.level_flow, b);
    lv.block_size = b;
    lv.lambda = (float)(B / 2) * (B / b);
    for (int m = 0; m < nm; ++m) {
        a.lambda_multiplier = mults[m];
        a.regularize_MVs();
        put_grid(lv.level_flow, b);
    }
    return 0;
}

static int cmd_search_from_coarse()
{
    std::vector<int> h = get_ints(2), search = get_ints(2), block = get_ints(2);
    int W = h[0], H = h[1];
    Mat f1(H, W, CV_8UC1), f2(H, W, CV_8UC1);
    get_plane(f1); get_plane(f2);
    MF a(f1, f2, search.data(), block.data(), 2);
    if (a.padding_x || a.padding_y || a.padded_width != W || a.padded_height != H) return 3;
    f1.copyTo(a.level_data[0].image1); f2.copyTo(a.level_data[0].image2);
    get_plane(a.level_data[1].image1); get_plane(a.level_data[1].image2);
    get_grid(a.level_data[1].level_flow, 2);
    a.curr_level = 0;
    a.copyMVs();
    a.calcLevelBM();
    put_grid(a.level_data[0].level_flow, block[0]);
    return 0;
}

static int cmd_mc()
{
    std::vector<int> h = get_ints(4);
    int W = h[0], H = h[1], b = h[2], fill = h[3], search = b;
    Mat f1 = Mat::zeros(H, W, CV_8UC1), f2(H, W, CV_8UC1);
    get_plane(f2);
    MF a(f1, f2, &search, &b, 1);
    if (a.padding_x || a.padding_y || a.padded_width != W || a.padded_height != H) return 3;
    a.curr_level = 0;
    get_grid(a.level_data[0].level_flow, b);
    Mat img(H, W, CV_8UC1, cv::Scalar(fill));
    a.draw_MVimage(img);
    put_plane(img);
    return 0;
}

static Mat get_flow(int W, int H)
{
    Mat m(H, W, CV_32FC2);
    for (int i = 0; i < H; ++i) get(m.data + (size_t)i * m.step, (size_t)W * 8);
    return m;
}

static int cmd_color()
{
    std::vector<int> h = get_ints(2);
    float maxmotion;
    get(&maxmotion, 4);
    Mat flow = get_flow(h[0], h[1]), img;
    Flow f;
    int keep = dup(1), nul = open("/dev/null", O_WRONLY);       // MotionToColor prints the motion range (:223)
    fflush(stdout); dup2(nul, 1);
    f.MotionToColor(flow, img, maxmotion);
    fflush(stdout); dup2(keep, 1);
    need(img.rows == h[1] && img.cols == h[0] && img.type() == CV_8UC3, "color: unexpected output image");
    for (int i = 0; i < img.rows; ++i) put(img.data + (size_t)i * img.step, (size_t)img.cols * 3);
    return 0;
}

static int cmd_mse()
{
    std::vector<int> h = get_ints(2);
    Mat gt = get_flow(h[0], h[1]), flow = get_flow(h[0], h[1]);
    Flow f;
    double e = f.CalculateMSE(gt, flow);
    put(&e, 8);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "plan")) return cmd_plan(argc, argv);
    int mode = 0, at = 2;
    if (argc >= 3 && !strcmp(argv[2], "--raster")) { mode = 1; at = 3; }
    else if (argc >= 3 && !strcmp(argv[2], "--parallel")) { mode = 2; at = 3; }
    if (argc != at + 2) {
        fprintf(stderr, "usage: mf_ref plan out L b.. w0 w1 h0 h1 | stages [--raster|--parallel] in out | sweeps in out |\n"
                        "       search-from-coarse in out | mc in out | color in out | mse in out\n");
        return 2;
    }
    g_in = fopen(argv[at], "rb");
    g_out = fopen(argv[at + 1], "wb");
    need(g_in && g_out, "cannot open the files");
    int rc = 2;
    std::string cmd = argv[1];
    if (cmd == "stages") rc = cmd_stages(mode);
    else if (cmd == "sweeps") rc = cmd_sweeps();
    else if (cmd == "search-from-coarse") rc = cmd_search_from_coarse();
    else if (cmd == "mc") rc = cmd_mc();
    else if (cmd == "color") rc = cmd_color();
    else if (cmd == "mse") rc = cmd_mse();
    else fprintf(stderr, "mf_ref: unknown command %s\n", argv[1]);
    if (rc == 0) need(fgetc(g_in) == EOF, "input file too long");
    fclose(g_out);
    return rc;
}
