"""Quarter-pel refinement (k_subpel_refine, the subpel rule of include/bbme.h) at the sizes a user runs:

  a   one pair's grid after the cfg3 estimate at 4K             bbme_subpel_device
  b   the statistics alone, with their download and wait        bbme_subpel_stats
  c   one pair's grid at the reference literals' native size    bbme_subpel_device (584 x 388, 4 levels, block 32, search 64)
  h   per size on the host: bbme_get_subpel_cells_host against the route without this kernel -- download two planes and the cells,
      then bbme_subpel_host --, alternating in one process
  p   per pair at the native size: estimate + refine + the field's download on a native context against the reference's route to
      sub-pixel vectors, an upsample=4 context on the same source (estimate at 16 x the pixels + the subsampled field's download)

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call; the lane-operations the rule needs by the kernel's own count (about 400 VALU per
candidate, 17 candidates per valid cell) and the rate that makes.  Kernel times come from a separate run under rocprofv3:

    python scripts/subpel_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/subpel_probe.py --reps 100 --host-reps 0 --pair-reps 0
    python scripts/subpel_probe.py --reps 100 --trace OUT      # k_subpel_refine dispatches per case (no GPU needed)
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

SIZES = {"4K": (3840, 2160, 80, 16, 4),                    # bench.py's cfg3
         "native": (584, 388, 64, 32, 4)}                  # the reference's literals on a Middlebury-sized frame, not enlarged
WARMUP = 10
VALU_PER_CELL = 17 * 400
CASES = [("a", "4K", "grid"), ("b", "4K", "stats"), ("c", "native", "grid")]


def _timed(fn, reps, stream):
    import torch
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
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in evs), statistics.median(wall) * 1e3


def run(reps, host_reps, pair_reps, device):
    import ctypes as C
    import numpy as np
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ctxs = {}
    for name, (w, h, search, block, levels) in SIZES.items():
        f1, f2, _ = bbme.synth_pair(w, h, 1030, max_motion=24 if name == "4K" else 8)
        mf = bbme.MF(f1, f2, [search] * levels, [block] * levels, levels, device=device)
        mf.estimate_async()
        mf.synchronize()
        handle = C.c_void_p()
        _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
        ch, cw = mf.cells_shape
        ctxs[name] = (mf, torch.cuda.ExternalStream(handle.value), torch.empty((ch, cw, 2), dtype=torch.int16, device="cuda:%d" % device),
                      (f1, f2))
        print("%s: %dx%d (padded %dx%d), search %d, block %d, %d levels: %d cells" % (name, w, h, mf.padded_width, mf.padded_height, search,
                                                                                    block, levels, ch * cw))
    print("%d calls per case after %d warm-up calls" % (reps, WARMUP))
    for name, size, what in CASES:
        mf, stream, out, _ = ctxs[size]
        ch, cw = mf.cells_shape
        if what == "grid":
            fn = lambda: _capi.check(mf._lib.bbme_subpel_device(mf._ctx, 0, 0, C.c_void_p(out.data_ptr()), cw, None))    # noqa: E731
        else:
            fn = lambda: mf.subpel_stats("forward", "all")                                                               # noqa: E731
        ev_ms, wall_ms = _timed(fn, reps, stream)
        valid = mf.subpel_stats("forward", "all")["valid"]
        ops = valid * VALU_PER_CELL
        print("  %s  %-6s %-5s: events %8.1f us, wall %8.1f us (medians); %d valid cells x %d VALU = %.2f G lane-operations -> %.1f T/s "
              "by the events" % (name, size, what, ev_ms * 1e3, wall_ms * 1e3, valid, VALU_PER_CELL, ops / 1e9, ops / (ev_ms * 1e-3) / 1e12))
    for size in SIZES if host_reps > 0 else ():
        mf = ctxs[size][0]
        gpu, route = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            q4 = mf.subpel_cells()
            gpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            p1, p2 = mf.get_level_planes(0)
            hq4, _ = bbme.subpel_cells(p1, p2, mf.get_cells())
            route.append(time.perf_counter() - t0)
        print("  h  %-6s one grid on the host, medians of %d alternating calls: bbme_get_subpel_cells_host %8.2f ms; two planes and the "
              "cells downloaded, then bbme_subpel_host %8.1f ms; equal: %s"
              % (size, host_reps, statistics.median(gpu) * 1e3, statistics.median(route) * 1e3, bool(np.array_equal(q4, hq4))))
    if pair_reps > 0:
        w, h, search, block, levels = SIZES["native"]
        mf, _, _, (f1, f2) = ctxs["native"]
        up = bbme.MF(f1, f2, [search] * levels, [block] * levels, levels, device=device, upsample=4)
        native, x4 = [], []
        for k in range(pair_reps + 2):
            t0 = time.perf_counter()
            mf.set_frames(f1, f2)
            mf.estimate_async()
            a = mf.subpel_flow()
            t1 = time.perf_counter()
            up.set_frames(f1, f2)
            up.estimate_async()
            b = up.get_subsampled_flow()
            t2 = time.perf_counter()
            if k >= 2:
                native.append(t1 - t0)
                x4.append(t2 - t1)
        print("  p  per pair at %dx%d, frames set, estimated and the %s field downloaded, medians of %d alternating pairs: native + "
              "refinement %8.2f ms; upsample=4 context (padded %dx%d) %8.2f ms; mean |difference| of the two fields %.3f px"
              % (w, h, a.shape, pair_reps, statistics.median(native) * 1e3, up.padded_width, up.padded_height, statistics.median(x4) * 1e3,
                 float(np.abs(a - b).mean())))
        up.close()
    for mf, _, _, _ in ctxs.values():
        mf.close()


def report(trace_dir, reps):
    """Durations of the k_subpel_refine dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_subpel_refine" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    expected = len(CASES) * (WARMUP + reps + 1)             # + the statistics call after each timed loop
    print("kernel times from %s: %d k_subpel_refine dispatches (%d expected)" % (os.path.relpath(f, trace_dir), len(dur), expected))
    if len(dur) != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0 --pair-reps 0)")
    for k, (name, size, what) in enumerate(CASES):
        timed = dur[k * (WARMUP + reps + 1) + WARMUP:k * (WARMUP + reps + 1) + WARMUP + reps]
        print("  %s  %-6s %-5s: kernel %7.1f us median (min %.1f, max %.1f)" % (name, size, what, statistics.median(timed), min(timed), max(timed)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pair-reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace", help="report the kernel times of a rocprofv3 --kernel-trace run of this probe")
    args = ap.parse_args()
    if args.trace:
        report(args.trace, args.reps)
    else:
        run(args.reps, args.host_reps, args.pair_reps, args.device)


if __name__ == "__main__":
    main()
