// bbme_main.cpp -- the reference's driver (main_class.cpp:6-85) as a real command line.
//
//   bbme_cli frame10.pgm|.ppm frame11.pgm|.ppm [--gt flow10.flo] [--out flow.flo] [--color flow.ppm] [--levels N]
//            [--block B] [--search S] [--no-upsample] [--device D] [--mc mc.pgm] [--backward back.flo] [--occlusion occ.pgm]
//            [--interpolate PREFIX --factor N] [--backward-color back.ppm] [--denoise PREFIX --strength T] [--subpel sub.flo]
//            [--mc-subpel mcq.pgm] [--interpolate-subpel PREFIX --factor N] [--denoise-subpel PREFIX --strength T]
//            [--global-motion [--gm-out gm.pgm] [--gm-out-bgr gm.ppm]]
//
// Sequence of main_class.cpp: read two grey frames (:24,26; binary PGM here, the image has no
// libpng), 4x bilinear up-sampling (:32-33) and MF::MF (:45) on the GPU from the original frames,
// timed calcMotionBlockMatching (:47-55) with the padding strip + every 4th pixel / 4 (:58-70) on
// the GPU, write the field (the reference only ever colour-codes it; here Flow::WriteFlowFile is
// actually called), EPE against ground truth (:78-82).  --mc writes the motion-compensated frame of draw_MVimage
// (motion_framework.cpp:887-905) with 2x2 blocks at level 0, the reference's "MC_imageL1" (:213-216), over the unpadded frame
// MF sees, and prints its PSNR against frame 1.  --backward writes the field from frame 2 to frame 1 (the context's direction
// BACKWARD, include/bbme.h) through the same subsampling and writer as --out; --occlusion writes the forward-backward consistency
// mask on frame 1 at tolerance 1, one byte per 2x2 cell whose top-left pixel lies in the unpadded frame MF sees (0 consistent,
// 128 inconsistent, 255 target outside the plane), and prints the three counts.  --interpolate PREFIX --factor N (default 2)
// writes the N - 1 frames between frame 1 and frame 2, phases k / N (the interpolation rule of include/bbme.h, from both fields),
// as PREFIX_k.pgm, each the unpadded frame MF sees.  --backward-color writes the colour coding (:73-75) of the backward field of a
// bidirectional estimate at the driver's subsampling; the image is made on the GPU from the cells (the colour rule of
// include/bbme.h) and only its bytes come back.  --color stays the host's Flow::MotionToColor of the downloaded field.
// --denoise PREFIX --strength T (default 64, 1..1021) writes PREFIX_1.pgm and PREFIX_2.pgm: each frame averaged with the other one,
// motion-aligned, where their 2x2 cells match better than T (the temporal filter rule of include/bbme.h, one neighbour each), as
// the unpadded frames; it needs --no-upsample (the frames written are the frames read; on colour frames, their luma).  On colour
// frames it also writes PREFIX_1.ppm and PREFIX_2.ppm: the colour frames filtered by the BGR temporal filter rule, whose weights
// come from the colour frames themselves (the largest per-channel 2x2 SAD) and not from the luma.
// --subpel writes the estimated field refined to quarter-pel on the planes the estimate ran on (the subpel rule of include/bbme.h),
// through the same writer as --out, and with --gt prints its EPE too: with --no-upsample sub-pixel vectors at the frames' own
// resolution, a sixteenth of the pixels of the reference's pipeline; without it sixteenths of a pixel of the frames read.
// --mc-subpel writes --mc's frame made along those quarter-pel vectors instead (the subpel compensation rule of include/bbme.h:
// bilinear quarter-pel samples of frame 2), the same unpadded crop, and prints the PSNR of both predictions against frame 1.
// On colour frames with --no-upsample (which keeps the colour) --mc and --mc-subpel also write the colour prediction (the BGR
// compensation rule of include/bbme.h along the integer and along the quarter-pel cells) beside the luma's, under the same name
// with .ppm in place of .pgm, and print its PSNR over the three channels next to the luma's.
// --interpolate-subpel PREFIX --factor N writes --interpolate's frames made at quarter-pel positions instead (the subpel
// interpolation rule of include/bbme.h: both fields refined to quarter-pel, every cell placed and sampled at its quarter-pel
// position of the phase), as PREFIX_k.pgm, the same unpadded crop; on colour frames the frames of their luma and, with
// --no-upsample (which keeps the colour), additionally PREFIX_k.ppm, colour frames by the BGR subpel interpolation rule.
// --denoise-subpel PREFIX --strength T writes --denoise's grey frames made along quarter-pel vectors instead (the subpel temporal
// filter rule of include/bbme.h: the field into the other frame refined to quarter-pel, its 2x2 cells sampled bilinearly), as
// PREFIX_1.pgm and PREFIX_2.pgm, the unpadded frames MF sees: with --no-upsample the frames read (on colour frames their luma),
// without it their 4x planes.  On colour frames with --no-upsample (which keeps the colour) additionally PREFIX_1.ppm and
// PREFIX_2.ppm, the colour frames by the BGR subpel temporal filter rule, as --denoise writes its own.
// --global-motion prints the dominant motion of the pair (the global motion rule of include/bbme.h: an affine model fitted to the
// estimated cells of the unpadded frame, tolerance one pixel, three iterations) as six numbers in pixels and pixels per pixel, the
// cells that follow it, that do not and that were excluded, and the PSNR of the prediction of frame 1 from frame 2 along the model
// alone (the global compensation rule) beside the block field's; --gm-out writes that prediction, the same unpadded crop as --mc.
// --gm-out-bgr, on .ppm frames with --no-upsample (which keeps the colour), writes the colour prediction (the BGR global
// compensation rule) and prints its PSNR over the three channels.
// Colour frames: binary PPM (P6, maxval 255) is accepted wherever PGM is (both frames of one kind).  Everything above is then
// computed from their luma (the luma rule of include/bbme.h) as for grey frames -- with --no-upsample the conversion runs on the
// GPU from the colour frames, otherwise on the host in front of the x4 up-sampling -- and --interpolate writes PREFIX_k.ppm,
// colour frames by the BGR interpolation rule; that needs --no-upsample (there is no up-sampled colour).
// Defaults are the reference's literals (:19-21): 4 levels, block 32, search 64.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>

#include "rw_flow.hpp"

// a binary PGM (P5) into `img`, or a binary PPM (P6; R,G,B per pixel in the file) into `bgr`; *colour tells which
static bool read_pnm(const char *path, bbme::Image8 &img, bbme::ImageBGR &bgr, bool *colour)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    char magic[3] = {0, 0, 0};
    int w = 0, h = 0, maxv = 0;
    auto skip = [&]() {
        int c;
        while ((c = fgetc(f)) != EOF) {
            if (c == '#') { while ((c = fgetc(f)) != EOF && c != '\n') {} }
            else if (c != ' ' && c != '\n' && c != '\r' && c != '\t') { ungetc(c, f); break; }
        }
    };
    bool ok = fread(magic, 1, 2, f) == 2 && magic[0] == 'P' && (magic[1] == '5' || magic[1] == '6');
    *colour = ok && magic[1] == '6';
    if (ok) { skip(); ok = fscanf(f, "%d", &w) == 1; }
    if (ok) { skip(); ok = fscanf(f, "%d", &h) == 1; }
    if (ok) { skip(); ok = fscanf(f, "%d", &maxv) == 1 && maxv == 255; }
    if (ok) ok = fgetc(f) != EOF && w > 0 && h > 0;
    if (ok && *colour) {
        bgr = bbme::ImageBGR(h, w);
        ok = fread(bgr.data.data(), 1, bgr.data.size(), f) == bgr.data.size();
        for (size_t i = 0; ok && i < bgr.data.size(); i += 3) std::swap(bgr.data[i], bgr.data[i + 2]);
    } else if (ok) {
        img = bbme::Image8(h, w);
        ok = fread(img.data.data(), 1, img.data.size(), f) == img.data.size();
    }
    fclose(f);
    return ok;
}

// the colour file that goes beside a grey one: the same name with .ppm in place of .pgm (or behind a name without it)
static std::string ppm_beside(const char *pgm)
{
    std::string name(pgm);
    if (name.size() >= 4 && name.compare(name.size() - 4, 4, ".pgm") == 0) name.resize(name.size() - 4);
    return name + ".ppm";
}

int main(int argc, char **argv)
{
    const char *f1 = nullptr, *f2 = nullptr, *gt = nullptr, *out = nullptr, *color = nullptr, *mc = nullptr, *backward = nullptr, *occlusion = nullptr, *interpolate = nullptr,
               *backward_color = nullptr, *denoise = nullptr, *subpel = nullptr, *mc_subpel = nullptr,
               *interpolate_subpel = nullptr, *denoise_subpel = nullptr, *gm_out = nullptr, *gm_out_bgr = nullptr;
    bool global_motion = false;
    int factor = 2, strength = 64;
    int levels = 4, block = 32, search = 64, device = 0;
    bool upsample = true;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a.c_str()); exit(2); } return argv[++i]; };
        if (a == "--gt") gt = next();
        else if (a == "--out") out = next();
        else if (a == "--color") color = next();
        else if (a == "--mc") mc = next();
        else if (a == "--mc-subpel") mc_subpel = next();
        else if (a == "--backward") backward = next();
        else if (a == "--occlusion") occlusion = next();
        else if (a == "--interpolate") interpolate = next();
        else if (a == "--interpolate-subpel") interpolate_subpel = next();
        else if (a == "--backward-color") backward_color = next();
        else if (a == "--denoise") denoise = next();
        else if (a == "--denoise-subpel") denoise_subpel = next();
        else if (a == "--subpel") subpel = next();
        else if (a == "--global-motion") global_motion = true;
        else if (a == "--gm-out") gm_out = next();
        else if (a == "--gm-out-bgr") gm_out_bgr = next();
        else if (a == "--strength") strength = atoi(next());
        else if (a == "--factor") factor = atoi(next());
        else if (a == "--levels") levels = atoi(next());
        else if (a == "--block") block = atoi(next());
        else if (a == "--search") search = atoi(next());
        else if (a == "--device") device = atoi(next());
        else if (a == "--no-upsample") upsample = false;
        else if (!f1) f1 = argv[i];
        else if (!f2) f2 = argv[i];
        else { fprintf(stderr, "unexpected argument %s\n", argv[i]); return 2; }
    }
    if (!f1 || !f2 || levels < 1 || levels > BBME_MAX_LEVELS || ((interpolate || interpolate_subpel) && (factor < 2 || factor > 256)) ||
        ((denoise || denoise_subpel) && (strength < 1 || strength > 1021))) {
        fprintf(stderr, "usage: bbme_cli frame1.pgm|.ppm frame2.pgm|.ppm [--gt gt.flo] [--out flow.flo] [--color flow.ppm] "
                        "[--levels N] [--block B] [--search S] [--no-upsample] [--device D] [--mc mc.pgm] [--backward back.flo] "
                        "[--occlusion occ.pgm] [--interpolate PREFIX --factor N] [--backward-color back.ppm] "
                        "[--denoise PREFIX --strength T] [--subpel sub.flo] [--mc-subpel mcq.pgm] "
                        "[--interpolate-subpel PREFIX --factor N] [--denoise-subpel PREFIX --strength T] "
                        "[--global-motion [--gm-out gm.pgm] [--gm-out-bgr gm.ppm]]\n"
                        "--denoise writes PREFIX_1.pgm and PREFIX_2.pgm (on .ppm frames their luma) and, on .ppm frames, the "
                        "filtered colour frames PREFIX_1.ppm and PREFIX_2.ppm; it needs --no-upsample\n");
        return 2;
    }
    if (denoise && upsample) {
        fprintf(stderr, "--denoise needs --no-upsample\n");
        return 2;
    }
    if (gm_out && !global_motion) {
        fprintf(stderr, "--gm-out needs --global-motion\n");
        return 2;
    }
    if (gm_out_bgr && (!global_motion || upsample)) {
        fprintf(stderr, "--gm-out-bgr needs --global-motion and --no-upsample\n");
        return 2;
    }
    try {
        bbme::Image8 image1, image2;
        bbme::ImageBGR bgr1, bgr2;
        bool colour = false, colour2 = false;
        if (!read_pnm(f1, image1, bgr1, &colour) || !read_pnm(f2, image2, bgr2, &colour2)) {
            fprintf(stderr, "Could not open one of the images\n");                    // main_class.cpp:40
            return 1;
        }
        if (colour != colour2) {
            fprintf(stderr, "One frame is grey (P5) and the other colour (P6): give two frames of one kind\n");
            return 1;
        }
        if (colour && upsample && interpolate) {
            fprintf(stderr, "--interpolate on colour frames needs --no-upsample\n");
            return 2;
        }
        if (gm_out_bgr && !colour) {
            fprintf(stderr, "--gm-out-bgr needs colour frames (.ppm)\n");
            return 2;
        }
        if (colour && upsample) { image1 = bbme::bgr_to_gray(bgr1); image2 = bbme::bgr_to_gray(bgr2); }
        const int scale = upsample ? 4 : 1;
        std::vector<int> search_size(levels, search), block_size(levels, block);
        // the x4 up-sampling (:32-33) runs on the GPU from the original frames; the padding strip and the every-4th-pixel / 4
        // subsampling (:58-70) too, so only the original-sized field comes back
        std::unique_ptr<MF> mf(colour && !upsample ? new MF(bgr1, bgr2, search_size.data(), block_size.data(), levels, device)
                                                   : new MF(image1, image2, search_size.data(), block_size.data(), levels, device, scale));
        MF &motion_pair = *mf;
        const auto t1 = std::chrono::steady_clock::now();
        bbme::ImageFlow subpix = motion_pair.calcMotionBlockMatchingSubsampled(scale);
        const auto t2 = std::chrono::steady_clock::now();
        printf("Seconds: %g\n", std::chrono::duration<double>(t2 - t1).count());
        Flow file;
        if (color) {                                   // main_class.cpp:73-75 (flow.png there)
            bbme::ImageBGR flow_img;
            file.MotionToColor(subpix, flow_img, -1);
            file.ShowImage(flow_img, color);
        }
        if (out) file.WriteFlowFile(subpix, out);
        if (gt) {
            bbme::ImageFlow gtruth;
            file.ReadFlowFile(gtruth, gt);
            printf("Calculated MSE is %.9g\n", file.CalculateMSE(gtruth, subpix));       // :82
        }
        if (subpel) {                                  // before anything below replaces the forward field
            const bbme::ImageFlow refined = motion_pair.subpelFlow();
            file.WriteFlowFile(refined, subpel);
            if (gt) {
                bbme::ImageFlow gtruth;
                file.ReadFlowFile(gtruth, gt);
                printf("Calculated MSE after quarter-pel refinement is %.9g\n", file.CalculateMSE(gtruth, refined));
            }
        }
        if (global_motion) {                           // before anything below replaces the forward field
            const MF::GlobalMotion g = motion_pair.globalMotion(BBME_GM_AFFINE, 65536, 3);
            const int W = motion_pair.padded_width, H = motion_pair.padded_height;
            // the model at the plane centre, and its slopes per pixel (two half pixels)
            printf("Global motion: u = %.6g %+.6g x %+.6g y, v = %.6g %+.6g x %+.6g y (pixels, x and y from the centre of the %dx%d "
                   "plane)\n", g.model[0] / 65536.0, g.model[1] / 32768.0, g.model[2] / 32768.0, g.model[3] / 65536.0,
                   g.model[4] / 32768.0, g.model[5] / 32768.0, W, H);
            printf("Global motion cells: %lld follow it, %lld do not, %lld excluded\n", g.words[0], g.words[1], g.words[2]);
            const bbme::CompensationError e = motion_pair.compensationError(0, 2), q = motion_pair.compensationErrorGlobal(g.model, 1);
            printf("Global MC PSNR is %.9g dB (block field: %.9g dB) over %llu pixels (%llu skipped)\n", q.psnr(), e.psnr(), q.pixels,
                   q.skipped);
            if (gm_out) {
                const bbme::Image8 img = motion_pair.drawMVimageGlobal(g.model, 1, false, 0);
                const int px = motion_pair.padding_x, py = motion_pair.padding_y;
                bbme::check(bbme_pgm_write(gm_out, img.cols - 2 * px, img.rows - 2 * py, img.cols,
                                           img.data.data() + (size_t)py * img.cols + px));
            }
            if (gm_out_bgr) {
                const bbme::ImageBGR img = motion_pair.drawMVimageGlobalBGR(g.model, 1, false, 0);
                bbme::check(bbme_ppm_write_bgr(gm_out_bgr, img.cols, img.rows, img.data.data()));
                const bbme::CompensationError c = motion_pair.compensationErrorGlobalBGR(g.model, 1);
                printf("Global MC colour PSNR is %.9g dB over %llu pixels (%llu skipped)\n", c.psnr(), c.pixels, c.skipped);
            }
        }
        if (mc) {
            const bbme::Image8 img = motion_pair.drawMVimage(0, 2, 0);
            const int px = motion_pair.padding_x, py = motion_pair.padding_y;
            bbme::check(bbme_pgm_write(mc, img.cols - 2 * px, img.rows - 2 * py, img.cols, img.data.data() + (size_t)py * img.cols + px));
            const bbme::CompensationError e = motion_pair.compensationError(0, 2);
            printf("MC PSNR is %.9g dB over %llu pixels (%llu skipped)\n", e.psnr(), e.pixels, e.skipped);
            if (colour && !upsample) {                 // the colour frame itself, by the BGR compensation rule along the integer cells
                const bbme::ImageBGR bgr = motion_pair.drawMVimageBGR(false, 0);
                bbme::check(bbme_ppm_write_bgr(ppm_beside(mc).c_str(), bgr.cols, bgr.rows, bgr.data.data()));
                const bbme::CompensationError c = motion_pair.compensationErrorBGR(1);
                printf("MC colour PSNR is %.9g dB over %llu pixels (%llu skipped)\n", c.psnr(), c.pixels, c.skipped);
            }
        }
        if (mc_subpel) {
            const bbme::Image8 img = motion_pair.drawMVimageSubpel(false, 0);
            const int px = motion_pair.padding_x, py = motion_pair.padding_y;
            bbme::check(bbme_pgm_write(mc_subpel, img.cols - 2 * px, img.rows - 2 * py, img.cols,
                                       img.data.data() + (size_t)py * img.cols + px));
            const bbme::CompensationError e = motion_pair.compensationError(0, 2), q = motion_pair.compensationErrorSubpel();
            printf("Quarter-pel MC PSNR is %.9g dB (integer vectors: %.9g dB) over %llu pixels (%llu skipped)\n", q.psnr(), e.psnr(),
                   q.pixels, q.skipped);
            if (colour && !upsample) {                 // the colour frame itself, by the BGR compensation rule along the quarter-pel cells
                const bbme::ImageBGR bgr = motion_pair.drawMVimageSubpelBGR(false, 0);
                bbme::check(bbme_ppm_write_bgr(ppm_beside(mc_subpel).c_str(), bgr.cols, bgr.rows, bgr.data.data()));
                const bbme::CompensationError c1 = motion_pair.compensationErrorBGR(1), c4 = motion_pair.compensationErrorBGR(4);
                printf("Quarter-pel MC colour PSNR is %.9g dB (integer vectors: %.9g dB) over %llu pixels (%llu skipped)\n", c4.psnr(),
                       c1.psnr(), c4.pixels, c4.skipped);
            }
        }
        if (backward) {
            // the subsampled getter reads the context's current field: estimate in direction BACKWARD, then back to FORWARD
            motion_pair.setDirection(true);
            file.WriteFlowFile(motion_pair.calcMotionBlockMatchingSubsampled(scale), backward);
            motion_pair.setDirection(false);
        }
        if (occlusion) {
            motion_pair.estimateBidirectional();
            bbme::Image8 mask = motion_pair.consistency(false, 1);
            for (uint8_t &v : mask.data) v = v == BBME_FB_CONSISTENT ? 0 : v == BBME_FB_INCONSISTENT ? 128 : 255;
            int win[4];
            motion_pair.unpaddedCells(win);
            bbme::check(bbme_pgm_write(occlusion, win[2], win[3], mask.cols, mask.data.data() + (size_t)win[1] * mask.cols + win[0]));
            const bbme::ConsistencyStats st = motion_pair.consistencyStats(false, 1);
            printf("consistent %llu inconsistent %llu outside %llu\n", st.consistent, st.inconsistent, st.outside);
        }
        if (interpolate) {
            motion_pair.estimateBidirectional();
            const int px = motion_pair.padding_x, py = motion_pair.padding_y;
            for (int k = 1; k < factor; ++k) {
                if (colour) {
                    const bbme::ImageBGR img = motion_pair.interpolateBGR(k, factor);
                    const std::string name = std::string(interpolate) + "_" + std::to_string(k) + ".ppm";
                    bbme::check(bbme_ppm_write_bgr(name.c_str(), img.cols, img.rows, img.data.data()));
                    continue;
                }
                const bbme::Image8 img = motion_pair.interpolate(k, factor);
                const std::string name = std::string(interpolate) + "_" + std::to_string(k) + ".pgm";
                bbme::check(bbme_pgm_write(name.c_str(), img.cols - 2 * px, img.rows - 2 * py, img.cols,
                                           img.data.data() + (size_t)py * img.cols + px));
            }
        }
        if (interpolate_subpel) {
            motion_pair.estimateBidirectional();
            const int px = motion_pair.padding_x, py = motion_pair.padding_y;
            for (int k = 1; k < factor; ++k) {
                const bbme::Image8 img = motion_pair.interpolateSubpel(k, factor);
                const std::string name = std::string(interpolate_subpel) + "_" + std::to_string(k) + ".pgm";
                bbme::check(bbme_pgm_write(name.c_str(), img.cols - 2 * px, img.rows - 2 * py, img.cols,
                                           img.data.data() + (size_t)py * img.cols + px));
                if (colour && !upsample) {
                    const bbme::ImageBGR bgr = motion_pair.interpolateSubpelBGR(k, factor);
                    const std::string ppm = std::string(interpolate_subpel) + "_" + std::to_string(k) + ".ppm";
                    bbme::check(bbme_ppm_write_bgr(ppm.c_str(), bgr.cols, bgr.rows, bgr.data.data()));
                }
            }
        }
        if (denoise) {
            motion_pair.estimateBidirectional();
            const int px = motion_pair.padding_x, py = motion_pair.padding_y;
            for (int which = 0; which < 2; ++which) {
                const bbme::Image8 img = motion_pair.temporalFilter(strength, which);
                const std::string name = std::string(denoise) + "_" + std::to_string(which + 1) + ".pgm";
                bbme::check(bbme_pgm_write(name.c_str(), img.cols - 2 * px, img.rows - 2 * py, img.cols,
                                           img.data.data() + (size_t)py * img.cols + px));
                if (colour) {                          // the colour frame itself, by the BGR temporal filter rule
                    const bbme::ImageBGR bgr = motion_pair.temporalFilterBgr(strength, which);
                    const std::string ppm = std::string(denoise) + "_" + std::to_string(which + 1) + ".ppm";
                    bbme::check(bbme_ppm_write_bgr(ppm.c_str(), bgr.cols, bgr.rows, bgr.data.data()));
                }
            }
        }
        if (denoise_subpel) {
            motion_pair.estimateBidirectional();
            const int px = motion_pair.padding_x, py = motion_pair.padding_y;
            for (int which = 0; which < 2; ++which) {
                const bbme::Image8 img = motion_pair.temporalFilterSubpel(strength, which);
                const std::string name = std::string(denoise_subpel) + "_" + std::to_string(which + 1) + ".pgm";
                bbme::check(bbme_pgm_write(name.c_str(), img.cols - 2 * px, img.rows - 2 * py, img.cols,
                                           img.data.data() + (size_t)py * img.cols + px));
                if (colour && !upsample) {             // the colour frame itself, by the BGR subpel temporal filter rule
                    const bbme::ImageBGR bgr = motion_pair.temporalFilterSubpelBgr(strength, which);
                    const std::string ppm = std::string(denoise_subpel) + "_" + std::to_string(which + 1) + ".ppm";
                    bbme::check(bbme_ppm_write_bgr(ppm.c_str(), bgr.cols, bgr.rows, bgr.data.data()));
                }
            }
        }
        if (backward_color) {
            motion_pair.estimateBidirectional();
            const bbme::ImageBGR img = motion_pair.flowColor(scale, -1.0f, true);
            bbme::check(bbme_ppm_write_bgr(backward_color, img.cols, img.rows, img.data.data()));
        }
    } catch (const bbme::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
