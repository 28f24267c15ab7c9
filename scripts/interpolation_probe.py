"""Motion-compensated interpolation (k_interpolate, the interpolation rule of include/bbme.h) at the size a user runs, after a
bidirectional estimate of the cfg3 4K pair:

  a   one phase, 1 / 2, frame                      bbme_interpolate_device
  b   a run of 3 phases, 1 / 4 .. 3 / 4, frames    bbme_interpolate_device, one launch
  c   6 pairs (2 distinct 4K pairs, each 3 times), statistics of all pairs in one launch   bbme_interpolation_stats
  h   the host route on the inputs of (a): download both planes and both grids, then bbme_interpolate_host

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call; the bytes the algorithm must move, computed from the shapes (both planes and both
grids once, every frame written once), and GB/s and the fraction of 8 TB/s.  (h): the median wall time per pair over
--host-reps calls.  Kernel times come from a separate run under rocprofv3:

    python scripts/interpolation_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/interpolation_probe.py --reps 100 --host-reps 0
    python scripts/interpolation_probe.py --reps 100 --trace OUT      # k_interpolate dispatches per case (no GPU needed)
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
BATCH, DISTINCT = 6, 2
# name, what the case computes, phases per launch, pairs per launch
CASES = [("a", "1 phase, frame", 1, 1), ("b", "3 phases, frames", 3, 1), ("c", "stats x6", 1, BATCH)]


def needed_bytes(pw, ph, phases, pairs, frames):
    """What the algorithm must move per call: both planes and both grids (one int16 pair per 2x2 cell) once per pair; every
    frame written once."""
    plane = pw * ph
    grid = (pw // 2) * (ph // 2) * 4
    return pairs * (2 * plane + 2 * grid) + (phases * plane if frames else 0)


def run(reps, host_reps, device):
    import ctypes as C
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    pairs = [bbme.synth_pair(W, H, 1000 + 30 + k, max_motion=24)[:2] for k in range(DISTINCT)]
    mf = bbme.MF(pairs[0][0], pairs[0][1], ss, bs, LEVELS, device=device)
    mf.estimate_bidirectional_async()
    mf.synchronize()
    pw, ph = mf.padded_width, mf.padded_height
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    out = torch.empty((3, ph, pw), dtype=torch.uint8, device="cuda:%d" % device)
    mb = bbme.MFBatch([pairs[k % DISTINCT] for k in range(BATCH)], ss, bs, LEVELS, device=device)
    mb.estimate_bidirectional_async()
    mb.synchronize()
    bhandle = C.c_void_p()
    _capi.check(mb._lib.bbme_get_stream(mb._ctx, C.byref(bhandle)))
    bstream = torch.cuda.ExternalStream(bhandle.value)

    def frames(num0, count, den):
        _capi.check(mf._lib.bbme_interpolate_device(mf._ctx, 0, num0, count, den, C.c_void_p(out.data_ptr()), pw, ph * pw, None))

    calls = {
        "a": (stream, lambda: frames(1, 1, 2)),
        "b": (stream, lambda: frames(1, 3, 4)),
        "c": (bstream, lambda: mb.interpolation_stats_all(1, 2)),
    }
    print("interpolation after bbme_estimate_bidirectional, cfg3 %dx%d (padded %dx%d), search %d, block %d, %d levels; "
          "%d calls per case after %d warm-up calls" % (W, H, pw, ph, SEARCH, BLOCK, LEVELS, reps, WARMUP))
    for name, what, phases, npairs in CASES:
        st, fn = calls[name]
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        wall = []
        for e0, e1 in evs:
            t0 = time.perf_counter()
            e0.record(st)
            fn()
            e1.record(st)
            e1.synchronize()
            wall.append(time.perf_counter() - t0)
        ev_ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in evs)
        nb = needed_bytes(pw, ph, phases, npairs, name != "c")
        print("  %s  %-17s: events %8.1f us, wall %8.1f us (medians); needs %6.1f MB -> %7.1f GB/s (%.3f of 8 TB/s) by the events"
              % (name, what, ev_ms * 1e3, statistics.median(wall) * 1e6, nb / 1e6, nb / (ev_ms * 1e-3) / 1e9,
                 nb / (ev_ms * 1e-3) / 1e9 / HBM_GBS))
    stats = mf.interpolation_stats(1, 2)
    print("  last values: %s" % (stats,))
    print("  pair 0 of the batch equals the single context: %s" % (mb.interpolation_stats_all(1, 2)[0] == stats,))
    if host_reps > 0:
        half = mf.interpolate(1, 2)
        wall = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            i1, i2 = mf.get_level_planes(0)
            f, b = mf.get_cells(), mf.get_backward_cells()
            frame, _, hstats = bbme.interpolate_cells(i1, i2, f, b, 1, 2, mf.default_cell_window())
            wall.append(time.perf_counter() - t0)
        print("  h  host route, 1 phase  : wall %8.1f ms per pair (median of %d): both planes and both grids downloaded (%.1f MB), "
              "then bbme_interpolate_host" % (statistics.median(wall) * 1e3, host_reps,
                                              (2 * pw * ph + 2 * (pw // 2) * (ph // 2) * 4) / 1e6))
        print("  the host route's frame and statistics equal the GPU's: %s" % (bool((frame == half).all()) and hstats == stats,))
    mb.close()
    mf.close()


def report(trace_dir, reps):
    """Durations of the k_interpolate dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_interpolate" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    expected = len(CASES) * (WARMUP + reps) + 2             # + the two statistics calls after the timed loops
    print("kernel times from %s: %d k_interpolate dispatches (%d expected)" % (os.path.relpath(f, trace_dir), len(dur), expected))
    if len(dur) != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0)")
    from blockbasedmotionestimation_amd.motion_framework import plan_padding
    pw, ph, _, _ = plan_padding(W, H, [SEARCH] * LEVELS, [BLOCK] * LEVELS)
    for k, (name, what, phases, npairs) in enumerate(CASES):
        timed = dur[k * (WARMUP + reps) + WARMUP:(k + 1) * (WARMUP + reps)]
        t = statistics.median(timed)
        nb = needed_bytes(pw, ph, phases, npairs, name != "c")
        print("  %s  %-17s: kernel %7.1f us median (min %.1f, max %.1f) -> %7.1f GB/s (%.3f of 8 TB/s)"
              % (name, what, t, min(timed), max(timed), nb / (t * 1e-6) / 1e9, nb / (t * 1e-6) / 1e9 / HBM_GBS))


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
