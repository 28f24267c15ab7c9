"""Temporal filter of colour frames (k_temporal_filter_bgr, the BGR temporal filter rule of include/bbme.h) at the size a user runs,
after a bidirectional estimate of a chain of three colour cfg3 4K frames (two pairs: one round of sequence.denoise_frames' plan):

  a   one two-sided frame (slot 1)                 bbme_temporal_filter_bgr_chain_device
  b   one one-sided frame (slot 0)                 bbme_temporal_filter_bgr_chain_device
  c   the round's three frames, one launch         bbme_temporal_filter_bgr_chain_device
  d   the statistics of every frame, one launch    bbme_temporal_filter_bgr_stats (with its download and wait)
  h   per frame on the host: bbme_get_temporal_filtered_bgr_host against the route without this kernel -- download three colour
      frames and two grids, then bbme_temporal_filter_bgr_host --, alternating in one process

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call; the bytes the algorithm must move, computed from the shapes (every colour frame, 3 W H
bytes, and every grid, W0 H0 bytes, the frames read once, every frame written once), and GB/s and the fraction of 8 TB/s.  Kernel
times come from a separate run under rocprofv3:

    python scripts/temporal_filter_bgr_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/temporal_filter_bgr_probe.py --reps 100 --host-reps 0
    python scripts/temporal_filter_bgr_probe.py --reps 100 --trace OUT      # k_temporal_filter_bgr dispatches per case (no GPU needed)
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

W, H, SEARCH, BLOCK, LEVELS = 3840, 2160, 80, 16, 4       # bench.py's cfg3
HBM_GBS = 8000.0
WARMUP = 10
STRENGTH = 64
# name, what the case computes, (colour frames, grids) it must move (frames and grids read once, frames written once)
CASES = [("a", "1 frame, two-sided", (3 + 1, 2)), ("b", "1 frame, one-sided", (2 + 1, 1)), ("c", "3 frames, one launch", (3 + 3, 4)),
         ("d", "stats of 3 frames", (3, 4))]


def case_bytes(objects, pw, ph):
    return objects[0] * 3 * W * H + objects[1] * pw * ph


def colour_video(bbme, frames):
    """Colour frames that move like synth_video's grey ones: three different pointwise maps of one video."""
    import numpy as np
    grey = bbme.synth_video(W, H, frames, 1030, max_motion=24)
    return [np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1)) for v in grey]


def run(reps, host_reps, device):
    import ctypes as C
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    video = colour_video(bbme, 3)
    mf = bbme.MFChain(video, ss, bs, LEVELS, device=device)
    mf.estimate_bidirectional_async()
    mf.synchronize()
    pw, ph = mf.padded_width, mf.padded_height
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    out = torch.empty((3, H, W, 3), dtype=torch.uint8, device="cuda:%d" % device)

    def frames(first, count):
        _capi.check(mf._lib.bbme_temporal_filter_bgr_chain_device(mf._ctx, first, count, STRENGTH, C.c_void_p(out.data_ptr()), 3 * W,
                                                                  3 * H * W, None))

    calls = {"a": lambda: frames(1, 1), "b": lambda: frames(0, 1), "c": lambda: frames(0, 3),
             "d": lambda: mf.temporal_filter_bgr_stats(STRENGTH)}
    print("colour temporal filter after bbme_estimate_bidirectional, chain of 3 colour cfg3 frames %dx%d (padded %dx%d), search %d, block %d, "
          "%d levels, strength %d; %d calls per case after %d warm-up calls" % (W, H, pw, ph, SEARCH, BLOCK, LEVELS, STRENGTH, reps, WARMUP))
    for name, what, objects in CASES:
        fn = calls[name]
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        wall = []
        for e0, e1 in evs:
            t0 = time.perf_counter()
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            wall.append(time.perf_counter() - t0)
        ev_ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in evs)
        nb = case_bytes(objects, pw, ph)
        print("  %s  %-21s: events %8.1f us, wall %8.1f us (medians); needs %6.1f MB -> %7.1f GB/s (%.3f of 8 TB/s) by the events"
              % (name, what, ev_ms * 1e3, statistics.median(wall) * 1e6, nb / 1e6, nb / (ev_ms * 1e-3) / 1e9,
                 nb / (ev_ms * 1e-3) / 1e9 / HBM_GBS))
    stats = mf.temporal_filter_bgr_stats(STRENGTH)
    print("  last values: %s" % (stats,))
    if host_reps > 0:
        gpu, route = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            frame = mf.get_frame_filtered_bgr(0, 1, STRENGTH)
            gpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            p, c, n = (mf.frame_bgr_tensor(q, w).cpu().numpy() for q, w in ((0, 0), (0, 1), (1, 1)))
            gp, gn = mf.get_pair_backward_cells(0), mf.get_pair_cells(1)
            hframe, _, hstats = bbme.temporal_filter_cells_bgr(c, p, n, gp, gn, STRENGTH, mf.padding_x, mf.padding_y,
                                                               mf.default_cell_window())
            route.append(time.perf_counter() - t0)
        print("  h  one two-sided frame on the host, medians of %d alternating calls: bbme_get_temporal_filtered_bgr_host %8.2f ms; "
              "three colour frames and two grids downloaded (%.1f MB), then bbme_temporal_filter_bgr_host %8.1f ms"
              % (host_reps, statistics.median(gpu) * 1e3, (9 * W * H + 2 * pw * ph) / 1e6, statistics.median(route) * 1e3))
        print("  the host route's frame and statistics equal the GPU's: %s"
              % (bool((frame == hframe).all()) and hstats == stats[1],))
    mf.close()


def report(trace_dir, reps):
    """Durations of the k_temporal_filter_bgr dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_temporal_filter_bgr" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    expected = len(CASES) * (WARMUP + reps) + 1             # + the statistics call after the timed loops
    print("kernel times from %s: %d k_temporal_filter_bgr dispatches (%d expected)" % (os.path.relpath(f, trace_dir), len(dur), expected))
    if len(dur) != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0)")
    from blockbasedmotionestimation_amd.motion_framework import plan_padding
    pw, ph, _, _ = plan_padding(W, H, [SEARCH] * LEVELS, [BLOCK] * LEVELS)
    for k, (name, what, objects) in enumerate(CASES):
        timed = dur[k * (WARMUP + reps) + WARMUP:(k + 1) * (WARMUP + reps)]
        t = statistics.median(timed)
        nb = case_bytes(objects, pw, ph)
        print("  %s  %-21s: kernel %7.1f us median (min %.1f, max %.1f); needs %6.1f MB -> %7.1f GB/s (%.3f of 8 TB/s)"
              % (name, what, t, min(timed), max(timed), nb / 1e6, nb / (t * 1e-6) / 1e9, nb / (t * 1e-6) / 1e9 / HBM_GBS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace", help="report the kernel times of a rocprofv3 --kernel-trace run of this probe")
    args = ap.parse_args()
    if args.trace:
        report(args.trace, args.reps)
    else:
        run(args.reps, args.host_reps, args.device)


if __name__ == "__main__":
    main()
