"""The colour temporal filter over two frames on each side (k_wide_temporal_filter_bgr; the BGR wide temporal filter rule of
include/bbme.h) at the size a user runs, after a bidirectional estimate of a COLOUR chain of five cfg3 4K frames, beside
k_wide_temporal_filter and k_subpel_temporal_filter_bgr on the same chain in the same run:

  b   one inner frame (slot 2), four neighbours         bbme_wide_temporal_filter_bgr_chain_device: 2 k_compose_cells + 4 k_subpel_refine
                                                        launches + the filter
  c   the chain's five frames, one filter launch        the same call: 2 k_compose_cells + 4 k_subpel_refine (3 or 4 grids each) + the filter
  d   the statistics of every frame alone               bbme_wide_temporal_filter_bgr_stats (with its download and wait)
  e   slot 2 by the grey wide filter (luma planes)      bbme_wide_temporal_filter_chain_device: the same grids + K15
  f   the five frames by the grey wide filter           the same call
  g   slot 2 by the colour subpel temporal filter       bbme_subpel_temporal_filter_bgr_chain_device: 2 k_subpel_refine launches + K13b
  i   the five frames by the colour subpel filter       the same call: 2 k_subpel_refine launches (4 pairs each) + K13b
  h   slot 2 on the host: bbme_get_wide_temporal_filtered_bgr_host against the route without this kernel -- download five colour
      frames, five luma planes and the integer grids, refine on the host, then bbme_wide_temporal_filter_bgr_host --, alternating
      in one process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, alternating (the order of the two swaps
      from run to run: parent, this, this, parent, ...), fresh processes

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call (composition and refinement launches included), and of the host wall time of the call.  Kernel times come from a separate run
under rocprofv3, with no counters beside it:

    python scripts/wide_temporal_filter_bgr_probe.py --reps 100 --host-reps 2
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/wide_temporal_filter_bgr_probe.py --reps 100 --host-reps 0
    python scripts/wide_temporal_filter_bgr_probe.py --reps 100 --trace OUT  # dispatches per case and kernel (no GPU needed)
    python scripts/wide_temporal_filter_bgr_probe.py --bench PARENT_CHECKOUT --bench-runs 3
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, SEARCH, BLOCK, LEVELS = 3840, 2160, 80, 16, 4       # bench.py's cfg3
FRAMES = 5
WARMUP = 5
STRENGTH = 64
# name, what the case computes, launches of one call: k_compose_cells, k_subpel_refine, k_wide_temporal_filter_bgr,
# k_wide_temporal_filter, k_subpel_temporal_filter_bgr
CASES = [("b", "colour wide, slot 2", (2, 4, 1, 0, 0)), ("c", "colour wide, 5 frames", (2, 4, 1, 0, 0)),
         ("d", "colour wide stats, 5", (2, 4, 1, 0, 0)), ("e", "grey wide, slot 2", (2, 4, 0, 1, 0)),
         ("f", "grey wide, 5 frames", (2, 4, 0, 1, 0)), ("g", "colour subpel, slot 2", (0, 2, 0, 0, 1)),
         ("i", "colour subpel, 5", (0, 2, 0, 0, 1))]
KERNELS = ("k_compose_cells", "k_subpel_refine", "k_wide_temporal_filter_bgr", "k_wide_temporal_filter", "k_subpel_temporal_filter_bgr")


def run(reps, host_reps, device):
    import ctypes as C
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    import numpy as np
    video = [np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))
             for v in bbme.synth_video(W, H, FRAMES, 1030, max_motion=24)]      # three pointwise maps of one grey video
    mf = bbme.MFChain(video, ss, bs, LEVELS, device=device)
    mf.estimate_bidirectional_async()
    mf.synchronize()
    pw, ph = mf.padded_width, mf.padded_height
    ch, cw = mf.cells_shape
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    out = torch.empty((FRAMES, max(ph * pw, 3 * H * W)), dtype=torch.uint8, device="cuda:%d" % device)
    last = {}

    def frames(call, first, count, colour):
        pitch = 3 * W if colour else pw
        _capi.check(call(mf._ctx, first, count, STRENGTH, C.c_void_p(out.data_ptr()), pitch, out.stride(0), None))

    def stats():
        last["d"] = mf.temporal_filter_wide_bgr_stats(STRENGTH)

    wide_bgr, wide, near_bgr = (mf._lib.bbme_wide_temporal_filter_bgr_chain_device, mf._lib.bbme_wide_temporal_filter_chain_device,
                                mf._lib.bbme_subpel_temporal_filter_bgr_chain_device)
    calls = {"b": lambda: frames(wide_bgr, 2, 1, True), "c": lambda: frames(wide_bgr, 0, FRAMES, True), "d": stats,
             "e": lambda: frames(wide, 2, 1, False), "f": lambda: frames(wide, 0, FRAMES, False),
             "g": lambda: frames(near_bgr, 2, 1, True), "i": lambda: frames(near_bgr, 0, FRAMES, True)}
    print("colour wide temporal filter after bbme_estimate_bidirectional, chain of %d cfg3 frames %dx%d (padded %dx%d, %dx%d cells), search %d, "
          "block %d, %d levels, strength %d; %d calls per case after %d warm-up calls"
          % (FRAMES, W, H, pw, ph, cw, ch, SEARCH, BLOCK, LEVELS, STRENGTH, reps, WARMUP))
    for name, what, _ in CASES:
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
        ev = [e0.elapsed_time(e1) * 1e3 for e0, e1 in evs]
        print("  %s  %-22s: events %8.1f us (min %.1f, max %.1f), wall %8.1f us (medians)"
              % (name, what, statistics.median(ev), min(ev), max(ev), statistics.median(wall) * 1e6))
    print("  last statistics: %s" % (last["d"],))
    if host_reps > 0:
        gpu, route = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            frame = mf.get_frame_filtered_wide_bgr(2, STRENGTH)
            gpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            p = [mf.get_slot_plane(0, s) for s in range(FRAMES)]
            col = [mf.frame_bgr_tensor(0, 0).cpu().numpy()] + [mf.frame_bgr_tensor(q, 1).cpu().numpy() for q in range(FRAMES - 1)]
            grids = [bbme.subpel_cells(p[2], p[n], g)[0] for n, g in ((1, mf.get_pair_backward_cells(1)), (3, mf.get_pair_cells(2)),
                                                                        (0, mf.composed_cells(2, -1)), (4, mf.composed_cells(2, 1)))]
            t1 = time.perf_counter()
            hframe, _, hstats = bbme.temporal_filter_cells_wide_bgr(col[2], [col[1], col[3], col[0], col[4]], grids, STRENGTH,
                                                                    mf.padding_x, mf.padding_y, mf.default_cell_window())
            route.append((t1 - t0, time.perf_counter() - t1))
        print("  h  slot 2 on the host, medians of %d alternating calls: bbme_get_wide_temporal_filtered_bgr_host %8.2f ms; five colour "
              "frames, five luma planes and four grids downloaded (%.1f MB) and refined by bbme_subpel_host %8.1f ms, then "
              "bbme_wide_temporal_filter_bgr_host %8.1f ms"
              % (host_reps, statistics.median(gpu) * 1e3, (5 * pw * ph + 15 * W * H + 16 * cw * ch) / 1e6,
                 statistics.median(r[0] for r in route) * 1e3, statistics.median(r[1] for r in route) * 1e3))
        print("  the host route's frame and statistics equal the GPU's: %s" % (bool((frame == hframe).all()) and hstats == last["d"][2],))
    mf.close()


def report(trace_dir, reps):
    """Durations of each kernel's dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    times = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
                 if re.search(r"(^|\W)%s(\W|$)" % k, r["Kernel_Name"])] for k in KERNELS}
    per = WARMUP + reps
    expected = tuple(sum(c[2][i] for c in CASES) * per for i in range(len(KERNELS)))
    found = tuple(len(times[k]) for k in KERNELS)
    print("kernel times from %s: dispatches of %s: %s (%s expected)" % (os.path.relpath(f, trace_dir), KERNELS, found, expected))
    if found != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0)")
    at = [0] * len(KERNELS)
    for name, what, launches in CASES:
        parts = []
        for i, k in enumerate(KERNELS):
            n = launches[i]
            if not n:
                continue
            t = times[k][at[i] + WARMUP * n:at[i] + per * n]
            at[i] += per * n
            per_call = [sum(t[j * n:(j + 1) * n]) for j in range(len(t) // n)]
            parts.append("%d %s %7.1f us a call (median; min %.1f, max %.1f)" % (n, k, statistics.median(per_call), min(per_call), max(per_call)))
        print("  %s  %-21s: %s" % (name, what, " | ".join(parts)))


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
    ap.add_argument("--host-reps", type=int, default=2)
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
