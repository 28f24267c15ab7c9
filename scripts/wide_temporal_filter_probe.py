"""Cell composition and the temporal filter over two frames on each side (k_compose_cells, k_wide_temporal_filter; the cell
composition rule and the wide temporal filter rule of include/bbme.h) at the size a user runs, after a bidirectional estimate of a
chain of five cfg3 4K frames, beside k_subpel_temporal_filter on the same chain in the same run:

  a   the composed grids into slot + 2 of slots 0 .. 2  bbme_compose_chain_device: 1 k_compose_cells launch
  b   one inner frame (slot 2), four neighbours         bbme_wide_temporal_filter_chain_device: 2 k_compose_cells + 4 k_subpel_refine
                                                        launches + the filter
  c   the chain's five frames, one filter launch        the same call: 2 k_compose_cells + 4 k_subpel_refine (3 or 4 grids each) + the filter
  d   the statistics of every frame alone               bbme_wide_temporal_filter_stats (with its download and wait)
  e   slot 2 by the subpel temporal filter              bbme_subpel_temporal_filter_chain_device: 2 k_subpel_refine launches + K13
  f   the five frames by the subpel temporal filter     the same call: 2 k_subpel_refine launches (4 pairs each) + K13
  h   slot 2 on the host: bbme_get_wide_temporal_filtered_host against the route without these kernels -- download five planes and
      four quarter-pel grids, then bbme_wide_temporal_filter_host --, alternating in one process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, alternating (the order of the two swaps
      from run to run: parent, this, this, parent, ...), fresh processes

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call (composition and refinement launches included), and of the host wall time of the call.  Kernel times come from a separate run
under rocprofv3, with no counters beside it:

    python scripts/wide_temporal_filter_probe.py --reps 50 --host-reps 2
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/wide_temporal_filter_probe.py --reps 50 --host-reps 0
    python scripts/wide_temporal_filter_probe.py --reps 50 --trace OUT       # dispatches per case and kernel (no GPU needed)
    python scripts/wide_temporal_filter_probe.py --bench PARENT_CHECKOUT --bench-runs 3
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
# name, what the case computes, launches of one call: k_compose_cells, k_subpel_refine, k_wide_temporal_filter, k_subpel_temporal_filter
CASES = [("a", "compose, 3 slots", (1, 0, 0, 0)), ("b", "wide, slot 2", (2, 4, 1, 0)), ("c", "wide, 5 frames", (2, 4, 1, 0)),
         ("d", "wide stats, 5 frames", (2, 4, 1, 0)), ("e", "subpel, slot 2", (0, 2, 0, 1)), ("f", "subpel, 5 frames", (0, 2, 0, 1))]
KERNELS = ("k_compose_cells", "k_subpel_refine", "k_wide_temporal_filter", "k_subpel_temporal_filter")


def run(reps, host_reps, device):
    import ctypes as C
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    video = bbme.synth_video(W, H, FRAMES, 1030, max_motion=24)
    mf = bbme.MFChain(video, ss, bs, LEVELS, device=device)
    mf.estimate_bidirectional_async()
    mf.synchronize()
    pw, ph = mf.padded_width, mf.padded_height
    ch, cw = mf.cells_shape
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    out = torch.empty((FRAMES, ph, pw), dtype=torch.uint8, device="cuda:%d" % device)
    cells = torch.empty((3, ch, cw, 2), dtype=torch.int16, device="cuda:%d" % device)
    last = {}

    def frames(call, first, count):
        _capi.check(call(mf._ctx, first, count, STRENGTH, C.c_void_p(out.data_ptr()), pw, ph * pw, None))

    def stats():
        last["d"] = mf.temporal_filter_wide_stats(STRENGTH)

    wide, near = mf._lib.bbme_wide_temporal_filter_chain_device, mf._lib.bbme_subpel_temporal_filter_chain_device
    calls = {"a": lambda: _capi.check(mf._lib.bbme_compose_chain_device(mf._ctx, 0, 3, 1, C.c_void_p(cells.data_ptr()), cw, ch * cw, None)),
             "b": lambda: frames(wide, 2, 1), "c": lambda: frames(wide, 0, FRAMES), "d": stats,
             "e": lambda: frames(near, 2, 1), "f": lambda: frames(near, 0, FRAMES)}
    print("wide temporal filter after bbme_estimate_bidirectional, chain of %d cfg3 frames %dx%d (padded %dx%d, %dx%d cells), search %d, "
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
        print("  %s  %-21s: events %8.1f us (min %.1f, max %.1f), wall %8.1f us (medians)"
              % (name, what, statistics.median(ev), min(ev), max(ev), statistics.median(wall) * 1e6))
    print("  last statistics: %s" % (last["d"],))
    if host_reps > 0:
        gpu, route = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            frame = mf.get_frame_filtered_wide(2, STRENGTH)
            gpu.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            p = [mf.get_slot_plane(0, s) for s in range(FRAMES)]
            grids = [bbme.subpel_cells(p[2], p[n], g)[0] for n, g in ((1, mf.get_pair_backward_cells(1)), (3, mf.get_pair_cells(2)),
                                                                        (0, mf.composed_cells(2, -1)), (4, mf.composed_cells(2, 1)))]
            t1 = time.perf_counter()
            hframe, _, hstats = bbme.temporal_filter_cells_wide(p[2], [p[1], p[3], p[0], p[4]], grids, STRENGTH, mf.default_cell_window())
            route.append((t1 - t0, time.perf_counter() - t1))
        print("  h  slot 2 on the host, medians of %d alternating calls: bbme_get_wide_temporal_filtered_host %8.2f ms; five planes and "
              "four grids downloaded (%.1f MB) and refined by bbme_subpel_host %8.1f ms, then bbme_wide_temporal_filter_host %8.1f ms"
              % (host_reps, statistics.median(gpu) * 1e3, (5 * pw * ph + 16 * cw * ch) / 1e6,
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
    expected = tuple(sum(c[2][i] for c in CASES) * per for i in range(4))
    found = tuple(len(times[k]) for k in KERNELS)
    print("kernel times from %s: dispatches of %s: %s (%s expected)" % (os.path.relpath(f, trace_dir), KERNELS, found, expected))
    if found != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0)")
    at = [0, 0, 0, 0]
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
    ap.add_argument("--reps", type=int, default=50)
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
