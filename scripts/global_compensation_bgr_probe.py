"""Colour global compensation (K18b k_global_compensate_bgr; the BGR global compensation rule of include/bbme.h) at 4K on a colour
context after the cfg3 bidirectional estimate, beside the kernels that move comparable bytes:

  a1  K18b, one frame                                            bbme_cells_global_compensate_bgr_device (d_out)
  a2  K18b, the statistics alone                                 bbme_cells_global_compensate_bgr_device (d_stats4)
  a3  K18b, both from one launch
  a4  K18b, a run of three frames under three models             bbme_cells_global_compensate_bgr_device (count = 3, d_out)
  b   K18 k_global_compensate on the luma planes, the frame      bbme_cells_global_compensate_device (d_out)
  c   K7b k_interpolate_bgr, one colour frame                    bbme_cells_interpolate_bgr_device (count = 1)
  h1  on the host clock: bbme_get_global_compensated_bgr_host against downloading both stored colour frames and running
      bbme_global_compensate_bgr_host, alternating in one process
  h2  sequence.stabilize_frames on a short 1080p colour video, per frame
  B   bench.py's `value` of this build and of a built checkout of the parent commit, the order swapping from run to run

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call.  Kernel times come from a separate run under rocprofv3:

    python scripts/global_compensation_bgr_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/global_compensation_bgr_probe.py --reps 100 --host-reps 0
    python scripts/global_compensation_bgr_probe.py --reps 100 --trace OUT      # the dispatches per case (no GPU needed)
    python scripts/global_compensation_bgr_probe.py --bench PARENT_CHECKOUT --bench-runs 3
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from global_motion_probe import SIZE, TOL, WARMUP, _timed, bench  # noqa: E402

# (case, kernel, what)
CASES = [("a1", "k_global_compensate_bgr", "frame"), ("a2", "k_global_compensate_bgr", "stats"), ("a3", "k_global_compensate_bgr", "both"),
         ("a4", "k_global_compensate_bgr", "3 frames"), ("b", "k_global_compensate", "luma"), ("c", "k_interpolate_bgr", "frame")]
VIDEO = (1920, 1080, 6)                                    # h2: width, height, frames


def _is(kernel, name):
    """A trace row's kernel name is `kernel`'s (k_global_compensate is a prefix of k_global_compensate_bgr)"""
    return kernel in name and (kernel != "k_global_compensate" or "k_global_compensate_bgr" not in name)


def _colour(grey):
    """Three pointwise maps of a grey frame as B,G,R"""
    import numpy as np
    return np.ascontiguousarray(np.stack([grey, 255 - grey, (grey.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))


def run(reps, host_reps, device):
    import numpy as np
    import torch
    import ctypes as C
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi, sequence
    w, h, search, block, levels = SIZE
    f1, f2, _ = bbme.synth_pair(w, h, 1030, max_motion=24)
    mf = bbme.MF(_colour(f1), _colour(f2), [search] * levels, [block] * levels, levels, device=device)
    mf.estimate_bidirectional_async()
    mf.synchronize()
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    dev = "cuda:%d" % device
    H0, W0 = mf.padded_height, mf.padded_width
    p2 = torch.from_numpy(mf.get_level_planes(0)[1]).to(dev)
    c1, c2 = mf.frame_bgr_tensor(0, 0), mf.frame_bgr_tensor(0, 1)
    fwd, bwd = mf.cells_tensor(0), mf.backward_cells_tensor(0)
    run3 = torch.stack([c2, c1, c2])
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    out3 = torch.empty((3, h, w, 3), dtype=torch.uint8, device=dev)
    plane = torch.empty((H0, W0), dtype=torch.uint8, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    mf.synchronize()
    got = mf.global_motion(tol=TOL, window="all")
    model = got["model"]
    models3 = np.stack([model, -model, model // 2]).astype(np.int32)
    print("4K colour: %dx%d (padded %dx%d, pads %d, %d), search %d, block %d, %d levels" % (w, h, W0, H0, mf.padding_x, mf.padding_y, search,
                                                                                           block, levels))
    print("model of the estimated field (affine, tol %d px, 3 iterations, all cells): %s" % (TOL, model.tolist()))
    print("%d calls per case after %d warm-up calls" % (reps, WARMUP))
    calls = {"a1": lambda: mf.cells_global_compensate_bgr_device(None, c2, model, out=out),
             "a2": lambda: mf.cells_global_compensate_bgr_device(c1, c2, model, stats=st),
             "a3": lambda: mf.cells_global_compensate_bgr_device(c1, c2, model, out=out, stats=st),
             "a4": lambda: mf.cells_global_compensate_bgr_device(None, run3, models3, out=out3),
             "b": lambda: mf.cells_global_compensate_device(None, p2, model, out=plane),
             "c": lambda: mf.cells_interpolate_bgr_device(fwd, bwd, out=out.unsqueeze(0))}
    for name, kernel, what in CASES:
        ev_ms, wall_ms = _timed(calls[name], reps, stream)
        print("  %-2s  %-24s %-9s: events %8.1f us, wall %8.1f us (medians)" % (name, kernel, what, ev_ms * 1e3, wall_ms * 1e3))
    e_grey, e_bgr = mf.compensation_error_global(model), mf.compensation_error_global_bgr(model)
    print("  prediction of the unpadded frame under the model: luma %.2f dB, colour %.2f dB over %d pixels (%d skipped)"
          % (e_grey["psnr"], e_bgr["psnr"], e_bgr["pixels"], e_bgr["skipped"]))
    gpu, route, same = [], [], True
    for _ in range(host_reps):
        t0 = time.perf_counter()
        a = mf.draw_MVimage_global_bgr(model)
        gpu.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b = bbme.global_compensate_bgr(None, c2.cpu().numpy(), model, 1, 0, mf.padding_x, mf.padding_y)[0]
        c1.cpu()
        route.append(time.perf_counter() - t0)
        same = same and np.array_equal(a, b)
    if host_reps > 0:
        print("  h1 one frame on the host clock, medians of %d alternating calls: bbme_get_global_compensated_bgr_host %8.2f ms; both "
              "colour frames downloaded (%.1f MB), then bbme_global_compensate_bgr_host %8.1f ms; equal: %s"
              % (host_reps, statistics.median(gpu) * 1e3, 2 * 3 * w * h / 1e6, statistics.median(route) * 1e3, same))
    mf.close()
    if host_reps > 0:
        vw, vh, n = VIDEO
        video = [_colour(f) for f in bbme.synth_video(vw, vh, n, 31, max_motion=6)]
        times = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            sequence.stabilize_frames(video, [search] * levels, [block] * levels, radius=1, device=device)
            times.append(time.perf_counter() - t0)
        print("  h2 stabilize_frames on %d colour frames of %dx%d, median of %d calls: %8.1f ms, %.1f ms per frame"
              % (n, vw, vh, host_reps, statistics.median(times) * 1e3, statistics.median(times) * 1e3 / n))


def report(trace_dir, reps):
    """Durations of each case's timed dispatches, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    print("kernel times from %s" % os.path.relpath(f, trace_dir))
    # dispatches behind the timed loops: the PSNR line's K18 and K18b
    tail = {"k_global_compensate_bgr": 1, "k_global_compensate": 1}
    for kernel in ("k_global_compensate_bgr", "k_global_compensate", "k_interpolate_bgr"):
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if _is(kernel, r["Kernel_Name"])]
        cases = [c for c in CASES if c[1] == kernel]
        if len(dur) != len(cases) * (WARMUP + reps) + tail.get(kernel, 0):
            raise SystemExit("%d %s dispatches, %d expected: not this probe's sequence (run it with --host-reps 0)"
                             % (len(dur), kernel, len(cases) * (WARMUP + reps) + tail.get(kernel, 0)))
        for k, (name, _, what) in enumerate(cases):
            timed = dur[k * (WARMUP + reps) + WARMUP:(k + 1) * (WARMUP + reps)]
            print("  %-2s  %-24s %-9s: kernel %7.1f us median (min %.1f, max %.1f) of %d" % (name, kernel, what,
                                                                                             statistics.median(timed), min(timed),
                                                                                             max(timed), len(timed)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace", help="report the kernel times of a rocprofv3 --kernel-trace run of this probe")
    ap.add_argument("--bench", metavar="PARENT", help="a built checkout of the parent commit: bench.py there and here, alternating")
    ap.add_argument("--bench-runs", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=3)
    args = ap.parse_args()
    if args.trace:
        report(args.trace, args.reps)
    elif args.bench:
        bench(os.path.abspath(args.bench), args.bench_runs, args.bench_steps, args.bench_warmup)
    else:
        run(args.reps, args.host_reps, args.device)


if __name__ == "__main__":
    main()
