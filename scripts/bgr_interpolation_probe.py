"""Colour video (the luma rule and the BGR interpolation rule of include/bbme.h) at the size a user runs, on the cfg3 4K pair
made colour (three pointwise maps of the grey frames) and after its bidirectional estimate:

  p   grey frames in HBM -> planes + pyramid       bbme_set_frames_device_pair   (k_pad_zero_run, the grey route's border copy)
  q   colour frames in HBM -> planes + pyramid     bbme_set_frames_device_bgr    (k_bgr_pad_run: convert + border + the kept copy)
  a   grey, one phase, 1 / 2                       bbme_interpolate_device       (k_interpolate)
  b   grey, a run of 3 phases, 1 / 4 .. 3 / 4      bbme_interpolate_device, one launch
  A   colour, one phase, 1 / 2                     bbme_interpolate_bgr_device   (k_interpolate_bgr)
  B   colour, a run of 3 phases                    bbme_interpolate_bgr_device, one launch
  h   the host route a user had before: download both luma planes, both grids and both colour frames, bbme_interpolate_bgr_host
  n   the new route: bbme_get_interpolated_bgr_host (the frame made on the GPU, only its bytes downloaded)

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call (p, q: the whole setter, cascade included), and of the host wall time of the call; the bytes the kernel must move, computed
from the shapes, GB/s and the share of the 3.8 TB/s k_fb_consistency reached.  h and n alternate in one process:
the median wall time per pair over --host-reps rounds.  Kernel times come from a separate run under rocprofv3:

    python scripts/bgr_interpolation_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/bgr_interpolation_probe.py --reps 100 --host-reps 0
    python scripts/bgr_interpolation_probe.py --reps 100 --trace OUT      # the kernels' dispatches per case (no GPU needed)
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
REF_GBS = 3800.0                                           # what k_fb_consistency reached
WARMUP = 10
# name, what the case does, the kernel it is about, phases per launch
CASES = [("p", "grey frames in", "k_pad_zero_run", 0), ("q", "colour frames in", "k_bgr_pad_run", 0),
         ("a", "grey, 1 phase", "k_interpolate", 1), ("b", "grey, 3 phases", "k_interpolate", 3),
         ("A", "colour, 1 phase", "k_interpolate_bgr", 1), ("B", "colour, 3 phases", "k_interpolate_bgr", 3)]


def needed_bytes(name, pw, ph, phases):
    """What the case's kernel must move per call.  p: both frames read, both planes written.  q: both colour frames read, both
    planes and both kept copies written.  a, b: both planes and both grids (one int16 pair per 2x2 cell) read, every frame
    written.  A, B: the same reads and both colour frames, every colour frame written."""
    plane, frame, grid = pw * ph, W * H, (pw // 2) * (ph // 2) * 4
    if name == "p":
        return 2 * frame + 2 * plane
    if name == "q":
        return 2 * 3 * frame + 2 * plane + 2 * 3 * frame
    if name in "ab":
        return 2 * plane + 2 * grid + phases * plane
    return 2 * plane + 2 * grid + 2 * 3 * frame + phases * 3 * frame


def colour_of(grey):
    import numpy as np
    return np.ascontiguousarray(np.stack([grey, 255 - grey, (grey.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))


def run(reps, host_reps, device):
    import ctypes as C
    import numpy as np
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    g1, g2 = bbme.synth_pair(W, H, 1000 + 30, max_motion=24)[:2]
    c1, c2 = colour_of(g1), colour_of(g2)
    y1, y2 = bbme.bgr_to_gray(c1), bbme.bgr_to_gray(c2)
    mf = bbme.MF(c1, c2, ss, bs, LEVELS, device=device)
    pw, ph = mf.padded_width, mf.padded_height
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    dev = "cuda:%d" % device
    ty1, ty2, tc1, tc2 = (torch.from_numpy(a).to(dev) for a in (y1, y2, c1, c2))
    out = torch.empty((3, ph, pw), dtype=torch.uint8, device=dev)
    out_bgr = torch.empty((3, H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def grey(num0, count, den):
        _capi.check(mf._lib.bbme_interpolate_device(mf._ctx, 0, num0, count, den, C.c_void_p(out.data_ptr()), pw, ph * pw, None))

    def colour(num0, count, den):
        _capi.check(mf._lib.bbme_interpolate_bgr_device(mf._ctx, 0, num0, count, den, C.c_void_p(out_bgr.data_ptr()), 3 * W,
                                                        3 * W * H, None))

    calls = {"p": lambda: mf.set_frames_device(ty1, ty2), "q": lambda: mf.set_frames_device(tc1, tc2),
             "a": lambda: grey(1, 1, 2), "b": lambda: grey(1, 3, 4), "A": lambda: colour(1, 1, 2), "B": lambda: colour(1, 3, 4)}
    print("colour frames in and out, cfg3 %dx%d (padded %dx%d), search %d, block %d, %d levels; %d calls per case after %d "
          "warm-up calls" % (W, H, pw, ph, SEARCH, BLOCK, LEVELS, reps, WARMUP))
    for name, what, kernel, phases in CASES:
        if name == "a":                                    # the setters are done: colour frames are in, estimate both ways
            mf.estimate_bidirectional_async()
            mf.synchronize()
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
        nb = needed_bytes(name, pw, ph, phases)
        print("  %s  %-17s: events %8.1f us, wall %8.1f us (medians); %s needs %6.1f MB%s"
              % (name, what, ev_ms * 1e3, statistics.median(wall) * 1e6, kernel, nb / 1e6,
                 "" if name in "pq" else " -> %7.1f GB/s (%.2f of 3.8 TB/s) by the events"
                 % (nb / (ev_ms * 1e-3) / 1e9, nb / (ev_ms * 1e-3) / 1e9 / REF_GBS)))
    if host_reps > 0:
        half = mf.interpolate_bgr(1, 2)
        px, py = mf.padding_x, mf.padding_y
        old, new = [], []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            i1, i2 = mf.get_level_planes(0)
            f, b = mf.get_cells(), mf.get_backward_cells()
            h1, h2 = tc1.cpu().numpy(), tc2.cpu().numpy()
            frame = bbme.interpolate_cells_bgr(i1, i2, h1, h2, f, b, 1, 2, px, py)
            old.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            mf.interpolate_bgr(1, 2, out=half)
            new.append(time.perf_counter() - t0)
        print("  h  host route, 1 phase  : wall %8.1f ms per pair (median of %d): planes, grids and colour downloaded (%.1f MB), "
              "then bbme_interpolate_bgr_host" % (statistics.median(old) * 1e3, host_reps,
                                                  (2 * pw * ph + 2 * (pw // 2) * (ph // 2) * 4 + 6 * W * H) / 1e6))
        print("  n  new route, 1 phase   : wall %8.1f ms per pair (median of %d, alternating with h): the frame from the GPU "
              "(%.1f MB downloaded)" % (statistics.median(new) * 1e3, host_reps, 3 * W * H / 1e6))
        print("  the host route's frame equals the GPU's: %s" % (bool(np.array_equal(frame, half)),))
    mf.close()


def report(trace_dir, reps):
    """Durations of each case's kernel over its timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))

    def family(name):
        for k in ("k_interpolate_bgr", "k_interpolate", "k_bgr_pad_run", "k_pad_zero_run"):
            if k in name:
                return k
        return None

    dur = {}
    for r in rows:
        dur.setdefault(family(r["Kernel_Name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    from blockbasedmotionestimation_amd.motion_framework import plan_padding
    pw, ph, _, _ = plan_padding(W, H, [SEARCH] * LEVELS, [BLOCK] * LEVELS)
    n = WARMUP + reps
    # the constructor's host setter is the first k_bgr_pad_run dispatch; a family's cases follow one another
    first = {"p": 0, "q": 1, "a": 0, "b": n, "A": 0, "B": n}
    print("kernel times from %s (run with --host-reps 0)" % os.path.relpath(f, trace_dir))
    for name, what, kernel, phases in CASES:
        d = dur.get(kernel, [])
        expected = {"k_pad_zero_run": n, "k_bgr_pad_run": n + 1}.get(kernel, 2 * n)
        if len(d) != expected:
            raise SystemExit("%d %s dispatches, %d expected: the trace does not hold the probe's sequence" % (len(d), kernel, expected))
        timed = d[first[name] + WARMUP:first[name] + n]
        t = statistics.median(timed)
        nb = needed_bytes(name, pw, ph, phases)
        print("  %s  %-17s: %-17s %7.1f us median (min %.1f, max %.1f); %6.1f MB -> %7.1f GB/s (%.2f of 3.8 TB/s)"
              % (name, what, kernel, t, min(timed), max(timed), nb / 1e6, nb / (t * 1e-6) / 1e9, nb / (t * 1e-6) / 1e9 / REF_GBS))


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
