// motion_framework.hpp -- C++ host-side mirror of the reference's MF class (motion_framework.h:9-54)
// over the C-ABI of libbbme.so.  Same class name, constructor argument order and public fields, so
// code written against the reference's MF compiles against this one after swapping cv::Mat for
// bbme::Image (or with -DBBME_WITH_OPENCV for the cv::Mat overloads).  Header only.
//
//   reference                                              here
//   MF(cv::Mat&, cv::Mat&, const int[], const int[], int)  MF(const Image8&, const Image8&, const int[], const int[], int)
//   cv::Mat calcMotionBlockMatching()                      ImageFlow calcMotionBlockMatching()
//   padded_height / padded_width / padding_x / padding_y   same public ints
//
// Errors: the reference asserts or prints and exit(1)s (motion_framework.cpp:7-8,21-26); this
// class throws bbme::Error carrying the C-ABI status and message.  Unlike the reference's MF, an
// instance may run calcMotionBlockMatching() any number of times (it is not one-shot).
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bbme.h"

#ifdef BBME_WITH_OPENCV
#include <opencv2/core/core.hpp>
#endif

namespace bbme {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &m) : std::runtime_error("bbme status " + std::to_string(s) + ": " + m), status(s) {}
};

inline void check(int status)
{
    if (status != BBME_OK) throw Error(status, bbme_last_error());
}

// 8-bit single-channel image (the reference's CV_8UC1 cv::Mat), row-major, pitch == cols
struct Image8 {
    int rows = 0, cols = 0;
    std::vector<uint8_t> data;
    Image8() = default;
    Image8(int r, int c) : rows(r), cols(c), data((size_t)r * c) {}
    uint8_t &at(int y, int x) { return data[(size_t)y * cols + x]; }
    uint8_t at(int y, int x) const { return data[(size_t)y * cols + x]; }
};

// two-band float image (the reference's CV_32FC2 cv::Mat): (u, v) = (dx, dy) interleaved
struct ImageFlow {
    int rows = 0, cols = 0;
    std::vector<float> data;
    ImageFlow() = default;
    ImageFlow(int r, int c) : rows(r), cols(c), data((size_t)r * c * 2) {}
    float *at(int y, int x) { return &data[2 * ((size_t)y * cols + x)]; }
    const float *at(int y, int x) const { return &data[2 * ((size_t)y * cols + x)]; }
};

// three-band 8-bit image, B,G,R interleaved (the reference's CV_8UC3 cv::Mat)
struct ImageBGR {
    int rows = 0, cols = 0;
    std::vector<uint8_t> data;
    ImageBGR() = default;
    ImageBGR(int r, int c) : rows(r), cols(c), data((size_t)r * c * 3) {}
    uint8_t *at(int y, int x) { return &data[3 * ((size_t)y * cols + x)]; }
    const uint8_t *at(int y, int x) const { return &data[3 * ((size_t)y * cols + x)]; }
};

// residual statistics of a motion-compensated frame (bbme_compensation_error)
struct CompensationError {
    unsigned long long sse = 0, sad = 0, pixels = 0, skipped = 0;
    int channels = 1;                                   // samples per pixel that sse and sad are summed over (3 for a colour rule)
    double mse() const { return pixels ? (double)sse / ((double)channels * (double)pixels) : std::numeric_limits<double>::quiet_NaN(); }
    // 10 log10(255^2 channels pixels / sse); infinite for a perfect prediction, NaN when no pixel was compensated
    double psnr() const
    {
        if (!pixels) return std::numeric_limits<double>::quiet_NaN();
        if (!sse) return std::numeric_limits<double>::infinity();
        return 10.0 * std::log10(255.0 * 255.0 * (double)channels * (double)pixels / (double)sse);
    }
};

// statistics of a forward-backward consistency mask (bbme_consistency_stats)
struct ConsistencyStats {
    unsigned long long consistent = 0, inconsistent = 0, outside = 0, discrepancy = 0;
};

// statistics of an interpolated frame (bbme_interpolation_stats): cells per selected hypothesis, the sum of their costs
struct InterpolationStats {
    unsigned long long forward = 0, backward = 0, zero = 0, cost = 0;
};

// cv::resize(img, img, cv::Size(), 4, 4, cv::INTER_LINEAR) of main_class.cpp:32-33
inline Image8 resize_x4(const Image8 &src)
{
    Image8 dst(src.rows * 4, src.cols * 4);
    check(bbme_resize_x4_host(src.data.data(), src.cols, src.rows, dst.data.data()));
    return dst;
}

// the luma of a B,G,R image (the luma rule of include/bbme.h)
inline Image8 bgr_to_gray(const ImageBGR &src)
{
    Image8 dst(src.rows, src.cols);
    check(bbme_bgr_to_gray_host(src.data.data(), src.cols, src.rows, 3 * src.cols, dst.data.data()));
    return dst;
}

}  // namespace bbme

class MF {
public:
    // upsample = 4: image1 / image2 are the ORIGINAL frames of the reference's pipeline; the context is created at their
    // x4 size (what the reference's MF sees after main_class.cpp:32-33) and the up-sampling runs on the GPU
    // (bbme_set_frames_host_x4).  padded_* / padding_* then describe the up-sampled frame.
    MF(const bbme::Image8 &image1, const bbme::Image8 &image2, const int search_size[], const int block_size[],
       const int num_levels, int device = 0, int upsample = 1)
        : upsample(upsample)
    {
        if (upsample != 1 && upsample != 4) throw bbme::Error(BBME_ERR_INVALID, "upsample must be 1 or 4");
        if (image1.rows != image2.rows || image1.cols != image2.cols)
            throw bbme::Error(BBME_ERR_INVALID, "image1.size() != image2.size()");                                 // assert :8
        create(image1.cols * upsample, image1.rows * upsample, search_size, block_size, num_levels, device);
        int rc = upsample == 4 ? bbme_set_frames_host_x4(ctx_, 0, image1.data.data(), image2.data.data(), image1.cols)
                               : bbme_set_frames_host(ctx_, image1.data.data(), image2.data.data(), image1.cols);
        if (rc != BBME_OK) { bbme_destroy(ctx_); ctx_ = nullptr; bbme::check(rc); }
    }
    // Colour frames, B,G,R (include/bbme.h: the luma rule makes the planes on the GPU, the context keeps the colour for
    // interpolateBGR); every estimate and result is the luma's.  There is no up-sampled form.
    MF(const bbme::ImageBGR &image1, const bbme::ImageBGR &image2, const int search_size[], const int block_size[],
       const int num_levels, int device = 0)
    {
        if (image1.rows != image2.rows || image1.cols != image2.cols)
            throw bbme::Error(BBME_ERR_INVALID, "image1.size() != image2.size()");
        create(image1.cols, image1.rows, search_size, block_size, num_levels, device);
        const int rc = bbme_set_frames_host_bgr(ctx_, 0, image1.data.data(), image2.data.data(), 3 * image1.cols);
        if (rc != BBME_OK) { bbme_destroy(ctx_); ctx_ = nullptr; bbme::check(rc); }
    }
#ifdef BBME_WITH_OPENCV
    MF(cv::Mat &image1, cv::Mat &image2, const int search_size[], const int block_size[], const int num_levels, int device = 0)
        : MF(from_mat(image1), from_mat(image2), search_size, block_size, num_levels, device) {}
#endif
    MF(const MF &) = delete;
    MF &operator=(const MF &) = delete;
    ~MF() { if (ctx_) bbme_destroy(ctx_); }

    // Perform block matching for the whole hierarchy/pyramid (motion_framework.cpp:113-219).
    // Returns the dense padded field (padded_height x padded_width, CV_32FC2 layout).
    bbme::ImageFlow calcMotionBlockMatching()
    {
        bbme::check(bbme_estimate(ctx_));
        bbme::ImageFlow flow(padded_height, padded_width);
        bbme::check(bbme_get_flow_host(ctx_, flow.data.data()));
        return flow;
    }
#ifdef BBME_WITH_OPENCV
    cv::Mat calcMotionBlockMatchingMat()
    {
        bbme::check(bbme_estimate(ctx_));
        cv::Mat flow(padded_height, padded_width, CV_32FC2);
        bbme::check(bbme_get_flow_host(ctx_, reinterpret_cast<float *>(flow.data)));
        return flow;
    }
#endif
    // calcMotionBlockMatching() followed by the driver's subsampling (main_class.cpp:58-70) on the GPU: the
    // ceil(W / scale) x ceil(H / scale) field of the unpadded frame at every scale-th pixel, divided by scale (scale 0 =
    // upsample, i.e. the original frame's size for an x4 MF).  Only that field is downloaded.
    bbme::ImageFlow calcMotionBlockMatchingSubsampled(int scale = 0)
    {
        if (scale == 0) scale = upsample;
        bbme::check(bbme_estimate(ctx_));
        int w = 0, h = 0;
        bbme::check(bbme_level_geometry(ctx_, 0, &w, &h, nullptr, nullptr));
        w -= 2 * padding_x;
        h -= 2 * padding_y;
        bbme::ImageFlow flow(scale > 0 ? (h + scale - 1) / scale : 0, scale > 0 ? (w + scale - 1) / scale : 0);
        bbme::check(bbme_get_subsampled_flow_host(ctx_, 0, scale, flow.data.data()));
        return flow;
    }
    // The current field refined to quarter-pel on the level-0 planes (the SUBPEL RULE of include/bbme.h), as the driver's field of
    // the source frame: every pixel its cell's quarter-pel vector / 4, or, on frames up-sampled x4, every 4th pixel / 16.
    // backward = true: the backward field after estimateBidirectional().  Needs an estimate.
    bbme::ImageFlow subpelFlow(bool backward = false)
    {
        int w = 0, h = 0;
        bbme::check(bbme_level_geometry(ctx_, 0, &w, &h, nullptr, nullptr));
        w -= 2 * padding_x;
        h -= 2 * padding_y;
        bbme::ImageFlow flow((h + upsample - 1) / upsample, (w + upsample - 1) / upsample);
        bbme::check(bbme_get_subpel_flow_host(ctx_, 0, backward ? 1 : 0, flow.data.data()));
        return flow;
    }
    // MF::draw_MVimage (motion_framework.cpp:887-905) from the level's current MV grid with b x b blocks (include/bbme.h):
    // the padded W_l x H_l plane, skipped blocks set to `fill`.  (level 0, block 2) after calcMotionBlockMatching is the
    // reference's "MC_imageL1" (:213-216).
    bbme::Image8 drawMVimage(int level = 0, int block = 2, int fill = 0)
    {
        int w = 0, h = 0;
        bbme::check(bbme_level_geometry(ctx_, level, &w, &h, nullptr, nullptr));
        bbme::Image8 img(h, w);
        bbme::check(bbme_get_motion_compensated_host(ctx_, 0, level, block, fill, img.data.data()));
        return img;
    }
    // The residual statistics of that frame against image1 over window {x0, y0, w, h} of the level plane; nullptr = the
    // unpadded frame at level 0, the whole plane at other levels.
    bbme::CompensationError compensationError(int level = 0, int block = 2, const int *window = nullptr)
    {
        int w = 0, h = 0;
        bbme::check(bbme_level_geometry(ctx_, level, &w, &h, nullptr, nullptr));
        const int unpadded[4] = {padding_x, padding_y, w - 2 * padding_x, h - 2 * padding_y};
        if (!window && level == 0) window = unpadded;
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_compensation_error(ctx_, level, block, window, s));
        bbme::CompensationError e;
        e.sse = s[0]; e.sad = s[1]; e.pixels = s[2]; e.skipped = s[3];
        return e;
    }
    // drawMVimage(0, 2) along the cells refined to quarter-pel (the SUBPEL COMPENSATION RULE of include/bbme.h): the padded level-0
    // plane; backward = image 2 predicted from image 1 along the backward cells of estimateBidirectional.
    bbme::Image8 drawMVimageSubpel(bool backward = false, int fill = 0)
    {
        int w = 0, h = 0;
        bbme::check(bbme_level_geometry(ctx_, 0, &w, &h, nullptr, nullptr));
        bbme::Image8 img(h, w);
        bbme::check(bbme_get_subpel_compensated_host(ctx_, 0, backward ? 1 : 0, fill, img.data.data()));
        return img;
    }
    // The residual statistics of that frame against the image it predicts over window {x0, y0, w, h} in pixels; nullptr = the
    // unpadded frame.
    bbme::CompensationError compensationErrorSubpel(bool backward = false, const int *window = nullptr)
    {
        int w = 0, h = 0;
        bbme::check(bbme_level_geometry(ctx_, 0, &w, &h, nullptr, nullptr));
        const int unpadded[4] = {padding_x, padding_y, w - 2 * padding_x, h - 2 * padding_y};
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_subpel_compensation_error(ctx_, backward ? 1 : 0, window ? window : unpadded, s));
        bbme::CompensationError e;
        e.sse = s[0]; e.sad = s[1]; e.pixels = s[2]; e.skipped = s[3];
        return e;
    }
    // The dominant motion of the current cells (the GLOBAL MOTION RULE of include/bbme.h) over the cells of the unpadded frame:
    // six Q16 integers in pixels (unit 1) over half pixels from the plane centre, and the sixteen words of the last moments pass
    // (words[0..2]: inliers, outliers, excluded).  tol_q16: the L1 tolerance in Q16 pixels.
    struct GlobalMotion { int32_t model[6]; long long words[16]; };
    GlobalMotion globalMotion(int kind = BBME_GM_AFFINE, long long tol_q16 = 65536, int iterations = 3, bool backward = false)
    {
        int win[4];
        unpaddedCells(win);
        GlobalMotion g{};
        bbme::check(bbme_global_motion(ctx_, backward ? 1 : 0, 0, kind, tol_q16, iterations, -1, win, g.model, g.words));
        return g;
    }
    // The class map of the current cells under that model: one byte (BBME_GM_*) per cell.
    bbme::Image8 globalMotionMap(const int32_t model[6], long long tol_q16 = 65536, bool backward = false)
    {
        bbme::Image8 map(padded_height / 2, padded_width / 2);
        bbme::check(bbme_get_global_motion_map_host(ctx_, 0, backward ? 1 : 0, 0, -1, model, tol_q16, map.data.data()));
        return map;
    }
    // The padded level-0 plane compensated for the model's motion alone (the GLOBAL COMPENSATION RULE of include/bbme.h), and its
    // residual statistics against the image it predicts over window {x0, y0, w, h} in pixels; nullptr = the unpadded frame.
    bbme::Image8 drawMVimageGlobal(const int32_t model[6], int unit = 1, bool backward = false, int fill = 0)
    {
        bbme::Image8 img(padded_height, padded_width);
        bbme::check(bbme_get_global_compensated_host(ctx_, 0, backward ? 1 : 0, model, unit, fill, img.data.data()));
        return img;
    }
    bbme::CompensationError compensationErrorGlobal(const int32_t model[6], int unit = 1, bool backward = false,
                                                    const int *window = nullptr)
    {
        const int unpadded[4] = {padding_x, padding_y, padded_width - 2 * padding_x, padded_height - 2 * padding_y};
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_global_compensation_error(ctx_, backward ? 1 : 0, model, unit, window ? window : unpadded, s));
        bbme::CompensationError e;
        e.sse = s[0]; e.sad = s[1]; e.pixels = s[2]; e.skipped = s[3];
        return e;
    }
    // The same in colour (the BGR GLOBAL COMPENSATION RULE of include/bbme.h), for frames set as B,G,R: the UNPADDED frame sampled
    // from the stored colour of the other image, and its statistics over window {x0, y0, w, h} in pixels of the frame (nullptr =
    // the whole frame), sse and sad summed over the three channels.
    bbme::ImageBGR drawMVimageGlobalBGR(const int32_t model[6], int unit = 1, bool backward = false, int fill = 0)
    {
        bbme::ImageBGR img(padded_height - 2 * padding_y, padded_width - 2 * padding_x);
        bbme::check(bbme_get_global_compensated_bgr_host(ctx_, 0, backward ? 1 : 0, model, unit, fill, img.data.data()));
        return img;
    }
    bbme::CompensationError compensationErrorGlobalBGR(const int32_t model[6], int unit = 1, bool backward = false,
                                                       const int *window = nullptr)
    {
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_global_compensation_error_bgr(ctx_, backward ? 1 : 0, model, unit, window, s));
        bbme::CompensationError e;
        e.sse = s[0]; e.sad = s[1]; e.pixels = s[2]; e.skipped = s[3]; e.channels = 3;
        return e;
    }
    // drawMVimage(0, 2) and drawMVimageSubpel in colour (the BGR COMPENSATION RULE of include/bbme.h, unit 1 and unit 4), for frames
    // set as B,G,R: the UNPADDED frame, every cell sampled from the stored colour of the other image along the integer cells or
    // along the cells refined to quarter pels on the luma planes; backward = frame 2 predicted from frame 1 along the backward cells
    // of estimateBidirectional.
    bbme::ImageBGR drawMVimageBGR(bool backward = false, int fill = 0) { return compensatedBGR(1, backward, fill); }
    bbme::ImageBGR drawMVimageSubpelBGR(bool backward = false, int fill = 0) { return compensatedBGR(4, backward, fill); }
    // The residual statistics of those frames (unit 1 or 4) against the colour frame they predict over window {x0, y0, w, h} in
    // pixels of the frame (nullptr = the whole frame), sse and sad summed over the three channels.
    bbme::CompensationError compensationErrorBGR(int unit, bool backward = false, const int *window = nullptr)
    {
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_compensation_error_bgr(ctx_, backward ? 1 : 0, unit, window, s));
        bbme::CompensationError e;
        e.sse = s[0]; e.sad = s[1]; e.pixels = s[2]; e.skipped = s[3]; e.channels = 3;
        return e;
    }
    // Direction of the context (include/bbme.h): backward = every estimate and result as if image1 and image2 were exchanged.
    void setDirection(bool backward) { bbme::check(bbme_set_direction(ctx_, backward ? BBME_DIR_BACKWARD : BBME_DIR_FORWARD)); }
    bool direction() const
    {
        int d = 0;
        bbme::check(bbme_get_direction(ctx_, &d));
        return d == BBME_DIR_BACKWARD;
    }
    // Backward and forward estimate of the pair from the planes the context holds; no host wait.  Leaves the direction forward.
    void estimateBidirectional() { bbme::check(bbme_estimate_bidirectional(ctx_)); }
    // The 2x2-cell grid of the forward (bbme_get_cells_host) / backward field: (padded_height / 2) x (padded_width / 2) (dx, dy) pairs.
    std::vector<int16_t> getCells()
    {
        std::vector<int16_t> cells((size_t)(padded_height / 2) * (padded_width / 2) * 2);
        bbme::check(bbme_get_cells_host(ctx_, cells.data()));
        return cells;
    }
    std::vector<int16_t> getBackwardCells()
    {
        std::vector<int16_t> cells((size_t)(padded_height / 2) * (padded_width / 2) * 2);
        bbme::check(bbme_get_backward_cells_host_pair(ctx_, 0, cells.data()));
        return cells;
    }
    // The consistency mask after estimateBidirectional(): one class byte (BBME_FB_*) per cell, on frame 1 (backward = false)
    // or on frame 2 (backward = true).
    bbme::Image8 consistency(bool backward = false, int tol = 1)
    {
        bbme::Image8 mask(padded_height / 2, padded_width / 2);
        bbme::check(bbme_get_consistency_host(ctx_, 0, backward ? BBME_DIR_BACKWARD : BBME_DIR_FORWARD, tol, mask.data.data()));
        return mask;
    }
    // The cells whose top-left pixel lies in the unpadded frame, {cx0, cy0, cw, ch}: the default window of consistencyStats.
    void unpaddedCells(int window[4]) const
    {
        const int w = padded_width - 2 * padding_x, h = padded_height - 2 * padding_y;
        window[0] = (padding_x + 1) / 2;
        window[1] = (padding_y + 1) / 2;
        window[2] = (padding_x + w + 1) / 2 - window[0];
        window[3] = (padding_y + h + 1) / 2 - window[1];
    }
    // Its statistics over window {cx0, cy0, cw, ch} in cells; nullptr = unpaddedCells.
    bbme::ConsistencyStats consistencyStats(bool backward = false, int tol = 1, const int *window = nullptr)
    {
        int unpadded[4];
        unpaddedCells(unpadded);
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_consistency_stats(ctx_, backward ? BBME_DIR_BACKWARD : BBME_DIR_FORWARD, tol, window ? window : unpadded, s));
        bbme::ConsistencyStats e;
        e.consistent = s[0]; e.inconsistent = s[1]; e.outside = s[2]; e.discrepancy = s[3];
        return e;
    }
    // The frame at phase num / den between image1 and image2 after estimateBidirectional() (the interpolation rule of
    // include/bbme.h): the padded plane; an upsample = 4 MF interpolates its 4x planes.
    bbme::Image8 interpolate(int num = 1, int den = 2)
    {
        bbme::Image8 img(padded_height, padded_width);
        bbme::check(bbme_get_interpolated_host(ctx_, 0, num, den, img.data.data()));
        return img;
    }
    // The same frame at quarter-pel positions (the subpel interpolation rule of include/bbme.h): both fields refined to quarter-pel,
    // every cell placed and sampled at its quarter-pel position of the phase; on an MF made of colour frames, of the luma planes.
    bbme::Image8 interpolateSubpel(int num = 1, int den = 2)
    {
        bbme::Image8 img(padded_height, padded_width);
        bbme::check(bbme_get_subpel_interpolated_host(ctx_, 0, num, den, img.data.data()));
        return img;
    }
    // Frame `which` (0 = image1, 1 = image2) averaged with the other frame, motion-aligned, where their 2x2 cells match better
    // than `strength` (the temporal filter rule of include/bbme.h) after estimateBidirectional(): the padded plane.
    bbme::Image8 temporalFilter(int strength, int which = 0)
    {
        bbme::Image8 img(padded_height, padded_width);
        bbme::check(bbme_get_temporal_filtered_host(ctx_, 0, which, strength, img.data.data()));
        return img;
    }
    // temporalFilter() along quarter-pel vectors (the subpel temporal filter rule of include/bbme.h): the cells the frame's
    // neighbour hangs on are refined and its 2x2 cells sampled bilinearly: the padded plane.
    bbme::Image8 temporalFilterSubpel(int strength, int which = 0)
    {
        bbme::Image8 img(padded_height, padded_width);
        bbme::check(bbme_get_subpel_temporal_filtered_host(ctx_, 0, which, strength, img.data.data()));
        return img;
    }
    // The same frame in colour (the BGR interpolation rule of include/bbme.h), for an MF made of colour frames: the UNPADDED frame.
    bbme::ImageBGR interpolateBGR(int num = 1, int den = 2)
    {
        bbme::ImageBGR img(padded_height - 2 * padding_y, padded_width - 2 * padding_x);
        bbme::check(bbme_get_interpolated_bgr_host(ctx_, 0, num, den, img.data.data()));
        return img;
    }
    // interpolateSubpel in colour (the BGR subpel interpolation rule of include/bbme.h), for an MF made of colour frames: the
    // quarter-pel selection on the luma planes, both colour frames sampled at the quarter-pel positions; the UNPADDED frame.
    bbme::ImageBGR interpolateSubpelBGR(int num = 1, int den = 2)
    {
        bbme::ImageBGR img(padded_height - 2 * padding_y, padded_width - 2 * padding_x);
        bbme::check(bbme_get_subpel_interpolated_bgr_host(ctx_, 0, num, den, img.data.data()));
        return img;
    }
    // temporalFilter in colour (the BGR temporal filter rule of include/bbme.h), for an MF made of colour frames: the stored
    // B,G,R frame `which` averaged with the other one where their 2x2 cells match better than `strength` in every channel;
    // the UNPADDED frame.
    bbme::ImageBGR temporalFilterBgr(int strength, int which = 0)
    {
        bbme::ImageBGR img(padded_height - 2 * padding_y, padded_width - 2 * padding_x);
        bbme::check(bbme_get_temporal_filtered_bgr_host(ctx_, 0, which, strength, img.data.data()));
        return img;
    }
    // temporalFilterBgr() along quarter-pel vectors (the BGR subpel temporal filter rule of include/bbme.h): the cells the frame's
    // neighbour hangs on are refined on the luma planes and its 2x2 colour cells sampled bilinearly; the UNPADDED frame.
    bbme::ImageBGR temporalFilterSubpelBgr(int strength, int which = 0)
    {
        bbme::ImageBGR img(padded_height - 2 * padding_y, padded_width - 2 * padding_x);
        bbme::check(bbme_get_subpel_temporal_filtered_bgr_host(ctx_, 0, which, strength, img.data.data()));
        return img;
    }
    // Its statistics over window {cx0, cy0, cw, ch} in cells; nullptr = unpaddedCells.
    bbme::InterpolationStats interpolationStats(int num = 1, int den = 2, const int *window = nullptr)
    {
        int unpadded[4];
        unpaddedCells(unpadded);
        unsigned long long s[4] = {0, 0, 0, 0};
        bbme::check(bbme_interpolation_stats(ctx_, num, den, window ? window : unpadded, s));
        bbme::InterpolationStats e;
        e.forward = s[0]; e.backward = s[1]; e.zero = s[2]; e.cost = s[3];
        return e;
    }
    // Flow::MotionToColor of the field calcMotionBlockMatchingSubsampled(scale) returns, on the GPU from the cells (the colour
    // rule of include/bbme.h): only the B,G,R image is downloaded.  backward = true: the backward field after
    // estimateBidirectional().  scale 0 = upsample; maxmotion > 0 replaces the normalising radius; range5, if given, receives
    // {max radius, min u, max u, min v, max v}.
    bbme::ImageBGR flowColor(int scale = 0, float maxmotion = -1.0f, bool backward = false, float *range5 = nullptr)
    {
        if (scale == 0) scale = upsample;
        const int w = padded_width - 2 * padding_x, h = padded_height - 2 * padding_y;
        bbme::ImageBGR img(scale > 0 ? (h + scale - 1) / scale : 0, scale > 0 ? (w + scale - 1) / scale : 0);
        bbme::check(bbme_get_flow_color_host(ctx_, 0, backward ? BBME_DIR_BACKWARD : BBME_DIR_FORWARD, scale, maxmotion,
                                             img.data.data(), range5));
        return img;
    }
    bbme_ctx *context() { return ctx_; }

    const int upsample = 1;       // 4: constructed from the original frames of the reference's x4 pipeline

    int padded_height = 0;        // motion_framework.h:16-19
    int padded_width = 0;
    int padding_x = 0;
    int padding_y = 0;

private:
    // MF::MF up to the frames: the context for width x height frames and the public geometry
    void create(int width, int height, const int search_size[], const int block_size[], int num_levels, int device)
    {
        if (num_levels <= 0) throw bbme::Error(BBME_ERR_INVALID, "num_levels must be > 0");                       // assert :7
        bbme_params p{};
        p.num_levels = num_levels;
        for (int i = 0; i < num_levels && i < BBME_MAX_LEVELS; ++i) {
            p.block_size[i] = block_size[i];
            p.search_size[i] = search_size[i];
        }
        bbme::check(bbme_create(&p, width, height, device, &ctx_));
        bbme::check(bbme_get_geometry(ctx_, &padded_width, &padded_height, &padding_x, &padding_y));
    }
    bbme::ImageBGR compensatedBGR(int unit, bool backward, int fill)
    {
        bbme::ImageBGR img(padded_height - 2 * padding_y, padded_width - 2 * padding_x);
        bbme::check(bbme_get_compensated_bgr_host(ctx_, 0, backward ? 1 : 0, unit, fill, img.data.data()));
        return img;
    }
#ifdef BBME_WITH_OPENCV
    static bbme::Image8 from_mat(const cv::Mat &m)
    {
        bbme::Image8 im(m.rows, m.cols);
        for (int y = 0; y < m.rows; ++y) std::copy(m.ptr<uint8_t>(y), m.ptr<uint8_t>(y) + m.cols, &im.data[(size_t)y * m.cols]);
        return im;
    }
#endif
    bbme_ctx *ctx_ = nullptr;
};
