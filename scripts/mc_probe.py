"""Motion compensation (k_motion_compensate: MF::draw_MVimage, motion_framework.cpp:887-905, with its residual statistics)
at the sizes a user runs, after a full bbme_estimate of the cfg3 4K pair:

  a   level 0, b = 2, statistics only        bbme_compensation_error
  b   level 0, b = 2, frame plus statistics  bbme_motion_compensate_device, then bbme_compensation_error
  c   level 0, b = 16, frame                 bbme_motion_compensate_device
  d   24 pairs (4 distinct 4K pairs, each 6 times), level 0, b = 2, statistics of all pairs in one call

Per case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call; the bytes the algorithm must move, computed from the shapes (image2, the
compensated frame and image1 once each, the 2x2 grid once), and GB/s and the fraction of 8 TB/s for both times.  Kernel
times come from a separate run under rocprofv3:

    python scripts/mc_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/mc_probe.py --reps 100
    python scripts/mc_probe.py --reps 100 --trace OUT      # k_motion_compensate dispatches per case (no GPU needed)
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
BATCH, DISTINCT = 24, 4
# name, level-0 block size, what the case computes, k_motion_compensate dispatches per call
CASES = [("a", 2, "stats", 1), ("b", 2, "frame+stats", 2), ("c", 16, "frame", 1), ("d", 2, "stats x24", 1)]


def needed_bytes(pw, ph, block, what, pairs=1):
    """What the algorithm must move per call: the grid (one int16 pair per 2x2 cell) and image2 once; the frame written
    once when asked for; image1 once when statistics are asked for."""
    plane = pw * ph
    grid = (pw // 2) * (ph // 2) * 4
    n = grid + plane                                       # grid + image2
    if "frame" in what:
        n += plane
    if "stats" in what:
        n += plane
    return n * pairs


def median_ms(ts):
    return statistics.median(ts) * 1e3


def run(reps, device):
    import torch
    import blockbasedmotionestimation_amd as bbme
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    f1, f2, _ = bbme.synth_pair(W, H, 1000 + 30, max_motion=24)
    mf = bbme.MF(f1, f2, ss, bs, LEVELS, device=device)
    mf.estimate_async()
    mf.synchronize()
    pw, ph = mf.padded_width, mf.padded_height
    import ctypes as C
    from blockbasedmotionestimation_amd import _capi
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    out = torch.empty((ph, pw), dtype=torch.uint8, device="cuda:%d" % device)
    pairs = [bbme.synth_pair(W, H, 1000 + 30 + k, max_motion=24)[:2] for k in range(DISTINCT)]
    mb = bbme.MFBatch([pairs[k % DISTINCT] for k in range(BATCH)], ss, bs, LEVELS, device=device)
    mb.estimate_async()
    mb.synchronize()
    bhandle = C.c_void_p()
    _capi.check(mb._lib.bbme_get_stream(mb._ctx, C.byref(bhandle)))
    bstream = torch.cuda.ExternalStream(bhandle.value)

    calls = {
        "a": (stream, lambda: mf.compensation_error(0, 2)),
        "b": (stream, lambda: (mf.motion_compensated_device(out, 0, 2), mf.compensation_error(0, 2))),
        "c": (stream, lambda: mf.motion_compensated_device(out, 0, 16)),
        "d": (bstream, lambda: mb.compensation_errors(0, 2)),
    }
    print("motion compensation after bbme_estimate, cfg3 %dx%d (padded %dx%d), search %d, block %d, %d levels; "
          "%d calls per case after %d warm-up calls" % (W, H, pw, ph, SEARCH, BLOCK, LEVELS, reps, WARMUP))
    results = {}
    for name, block, what, _ in CASES:
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
        nb = needed_bytes(pw, ph, block, what, BATCH if name == "d" else 1)
        results[name] = (ev_ms, median_ms(wall), nb)
        print("  %s  level 0, b = %2d, %-11s: events %8.1f us, wall %8.1f us (medians); needs %6.1f MB -> %7.1f GB/s "
              "(%.3f of 8 TB/s) by the events" % (name, block, what, ev_ms * 1e3, median_ms(wall) * 1e3, nb / 1e6,
                                                   nb / (ev_ms * 1e-3) / 1e9, nb / (ev_ms * 1e-3) / 1e9 / HBM_GBS))
    a, b = results["a"], results["b"]
    print("  stats of the 24 pairs per pair: %.1f us (events)" % (results["d"][0] * 1e3 / BATCH))
    print("  last values: %s" % (mf.compensation_error(0, 2),))
    print("  pair 0 of the batch equals the single context: %s" % (mb.compensation_errors(0, 2)[0] == mf.compensation_error(0, 2),))
    print("  (a) and (b) events medians: %.1f / %.1f us" % (a[0] * 1e3, b[0] * 1e3))
    mb.close()
    mf.close()


def report(trace_dir, reps):
    """Durations of the k_motion_compensate dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted((r for r in csv.DictReader(open(f)) if "k_motion_compensate" in r["Kernel_Name"]),
                  key=lambda r: int(r["Start_Timestamp"]))
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    expected = sum((WARMUP + reps) * n for _, _, _, n in CASES) + 3     # + the three calls after the timed loops
    print("kernel times from %s: %d k_motion_compensate dispatches (%d expected)" % (os.path.relpath(f, trace_dir), len(dur),
                                                                                  expected))
    if len(dur) != expected:
        raise SystemExit("the trace does not hold the probe's dispatch sequence")
    at = 0
    from blockbasedmotionestimation_amd.motion_framework import plan_padding
    pw, ph, _, _ = plan_padding(W, H, [SEARCH] * LEVELS, [BLOCK] * LEVELS)
    for name, block, what, n in CASES:
        timed = dur[at + WARMUP * n:at + (WARMUP + reps) * n]
        at += (WARMUP + reps) * n
        per_kind = [statistics.median(timed[k::n]) for k in range(n)]
        tot = sum(per_kind)
        nb = needed_bytes(pw, ph, block, what, BATCH if name == "d" else 1)
        print("  %s  level 0, b = %2d, %-11s: kernel %s us median%s -> %7.1f GB/s (%.3f of 8 TB/s)"
              % (name, block, what, " + ".join("%.1f" % t for t in per_kind), " (frame pass + stats pass)" if n == 2 else "",
                 nb / (tot * 1e-6) / 1e9, nb / (tot * 1e-6) / 1e9 / HBM_GBS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace", help="report the kernel times of a rocprofv3 --kernel-trace run of this probe")
    args = ap.parse_args()
    if args.trace:
        report(args.trace, args.reps)
    else:
        run(args.reps, args.device)


if __name__ == "__main__":
    main()
