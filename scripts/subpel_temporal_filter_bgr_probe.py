"""Temporal filter of colour frames along quarter-pel grids (k_subpel_temporal_filter_bgr, the BGR subpel temporal filter rule of
include/bbme.h) at the size a user runs, after a bidirectional estimate of a chain of three colour cfg3 4K frames (two pairs: one
round of sequence.denoise_frames' default plan), beside k_temporal_filter_bgr on the integer grids and k_subpel_temporal_filter on
the luma planes of the same estimate in the same run:

  a   one two-sided frame (slot 1)                 bbme_subpel_temporal_filter_bgr_chain_device: 2 k_subpel_refine launches + the filter
  b   one one-sided frame (slot 0)                 the same call: 1 k_subpel_refine launch + the filter
  c   the round's three frames, one launch         the same call: 2 k_subpel_refine launches (2 pairs each) + the filter
  d   the statistics of every frame, one launch    bbme_subpel_temporal_filter_bgr_stats (with its download and wait)
  the same four of the integer colour filter (bbme_temporal_filter_bgr_chain_device, bbme_temporal_filter_bgr_stats) and of the grey
  quarter-pel filter (bbme_subpel_temporal_filter_chain_device, bbme_subpel_temporal_filter_stats)
  h   per frame on the host: bbme_get_subpel_temporal_filtered_bgr_host against the route without this kernel -- download three
      colour frames and two quarter-pel grids, then bbme_subpel_temporal_filter_bgr_host --, alternating in one process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, alternating (the order of the two swaps
      from run to run: parent, this, this, parent, ...), fresh processes

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call (refinement launches included), and of the host wall time of the call.  Kernel times come from a separate run under rocprofv3:

    python scripts/subpel_temporal_filter_bgr_probe.py --reps 100 --host-reps 3
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/subpel_temporal_filter_bgr_probe.py --reps 100 --host-reps 0
    python scripts/subpel_temporal_filter_bgr_probe.py --reps 100 --trace OUT      # dispatches per case and kernel (no GPU needed)
    python scripts/subpel_temporal_filter_bgr_probe.py --bench PARENT_CHECKOUT --bench-runs 3
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SEARCH, BLOCK, LEVELS = 3840, 2160, 80, 16, 4       # bench.py's cfg3
WARMUP = 10
STRENGTH = 64
# name, what the case computes, k_subpel_refine launches of one quarter-pel call
CASES = [("a", "1 frame, two-sided", 2), ("b", "1 frame, one-sided", 1), ("c", "3 frames, one launch", 2), ("d", "stats of 3 frames", 2)]
# the flavours a case runs, in this order: name, kernel, whether its calls refine
FLAVOURS = [("quarter-pel colour", "k_subpel_temporal_filter_bgr", True), ("integer colour", "k_temporal_filter_bgr", False),
            ("quarter-pel grey", "k_subpel_temporal_filter", True)]


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
    plane = torch.empty((3, ph, pw), dtype=torch.uint8, device="cuda:%d" % device)
    L = mf._lib
    chain_calls = [L.bbme_subpel_temporal_filter_bgr_chain_device, L.bbme_temporal_filter_bgr_chain_device,
                   L.bbme_subpel_temporal_filter_chain_device]
    stats_calls = [mf.temporal_filter_subpel_bgr_stats, mf.temporal_filter_bgr_stats, mf.temporal_filter_subpel_stats]

    def frames(flavour, first, count):
        if flavour == 2:
            _capi.check(chain_calls[2](mf._ctx, first, count, STRENGTH, C.c_void_p(plane.data_ptr()), pw, ph * pw, None))
        else:
            _capi.check(chain_calls[flavour](mf._ctx, first, count, STRENGTH, C.c_void_p(out.data_ptr()), 3 * W, 3 * H * W, None))

    def calls(flavour):
        return {"a": lambda: frames(flavour, 1, 1), "b": lambda: frames(flavour, 0, 1), "c": lambda: frames(flavour, 0, 3),
                "d": lambda: stats_calls[flavour](STRENGTH)}

    print("colour subpel temporal filter after bbme_estimate_bidirectional, chain of 3 colour cfg3 frames %dx%d (padded %dx%d), search "
          "%d, block %d, %d levels, strength %d; %d calls per case after %d warm-up calls"
          % (W, H, pw, ph, SEARCH, BLOCK, LEVELS, STRENGTH, reps, WARMUP))
    for name, what, _ in CASES:
        for flavour, (label, _, _) in enumerate(FLAVOURS):
            fn = calls(flavour)[name]
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
            print("  %s  %-21s %-18s: events %8.1f us, wall %8.1f us (medians)"
                  % (name, what, label, ev_ms * 1e3, statistics.median(wall) * 1e6), flush=True)
    stats = mf.temporal_filter_subpel_bgr_stats(STRENGTH)
    print("  last values: %s" % (stats,))
    print("  integer colour rule: %s" % (mf.temporal_filter_bgr_stats(STRENGTH),))
    if host_reps > 0:
        gpu, route = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            frame = mf.get_frame_filtered_subpel_bgr(0, 1, STRENGTH)
            gpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            p, c, n = (mf.frame_bgr_tensor(q, w).cpu().numpy() for q, w in ((0, 0), (0, 1), (1, 1)))
            qp, qn = mf.get_pair_subpel_cells(0, "backward"), mf.get_pair_subpel_cells(1, "forward")
            hframe, _, hstats = bbme.temporal_filter_cells_subpel_bgr(c, p, n, qp, qn, STRENGTH, mf.padding_x, mf.padding_y,
                                                                      mf.default_cell_window())
            route.append(time.perf_counter() - t0)
        print("  h  one two-sided frame on the host, medians of %d alternating calls: bbme_get_subpel_temporal_filtered_bgr_host %8.2f ms; "
              "three colour frames and two quarter-pel grids downloaded (%.1f MB), then bbme_subpel_temporal_filter_bgr_host %8.1f ms"
              % (host_reps, statistics.median(gpu) * 1e3, (9 * W * H + 2 * pw * ph) / 1e6, statistics.median(route) * 1e3))
        print("  the host route's frame and statistics equal the GPU's: %s" % (bool((frame == hframe).all()) and hstats == stats[1],))
    mf.close()


def report(trace_dir, reps):
    """Durations of the filter and refinement dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))

    def durations(pick):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if pick(r["Kernel_Name"])]

    times = [durations(lambda n: "k_subpel_temporal_filter_bgr" in n),
             durations(lambda n: "k_temporal_filter_bgr" in n and "subpel" not in n),
             durations(lambda n: "k_subpel_temporal_filter" in n and "k_subpel_temporal_filter_bgr" not in n)]
    refine = durations(lambda n: "k_subpel_refine" in n)
    per = WARMUP + reps
    # the two closing statistics calls add one dispatch of the two colour kernels and two refinement launches
    expected = (len(CASES) * per + 1, len(CASES) * per + 1, len(CASES) * per, 2 * sum(n for _, _, n in CASES) * per + 2)
    print("kernel times from %s: %s dispatches of the three filters, %d k_subpel_refine dispatches (%s expected)"
          % (os.path.relpath(f, trace_dir), [len(t) for t in times], len(refine), expected))
    if tuple(len(t) for t in times) + (len(refine),) != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0)")
    for k, (name, what, launches) in enumerate(CASES):
        med = []
        for (label, kernel, _), t in zip(FLAVOURS, times):
            t = t[k * per + WARMUP:(k + 1) * per]
            med.append(statistics.median(t))
            print("  %s  %-21s: %-28s %7.1f us median (min %.1f, max %.1f)" % (name, what, kernel, med[-1], min(t), max(t)))
        print("  %s  %-21s: ratio to k_temporal_filter_bgr %.2f, to k_subpel_temporal_filter %.2f; %d k_subpel_refine launches a call"
              % (name, what, med[0] / med[1], med[0] / med[2], launches))
    print("  k_subpel_refine: %7.1f us median over all %d dispatches" % (statistics.median(refine), len(refine)))


def bench(parent, runs, steps, warmup):
    """bench.py of this tree and of the parent's checkout, a fresh process each, the order of the two swapping from run to run:
    every `value` and the ranges"""
    values = {"this": [], "parent": []}
    for n in range(runs):
        order = (("parent", parent), ("this", ROOT))
        for name, root in order[::-1] if n % 2 else order:
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=root, capture_output=True, text=True, check=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            values[name].append(json.loads(line)["value"])
            print("  B  %-6s value %s" % (name, values[name][-1]), flush=True)
    for name, v in values.items():
        print("  B  %-6s median %.4f (min %.4f, max %.4f) of %d runs" % (name, statistics.median(v), min(v), max(v), len(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace", help="report the kernel times of a rocprofv3 --kernel-trace run of this probe")
    ap.add_argument("--bench", metavar="PARENT", help="a built checkout of the parent commit: bench.py there and here, alternating")
    ap.add_argument("--bench-runs", type=int, default=3)
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
