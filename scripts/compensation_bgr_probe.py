"""Colour motion compensation along the cells (K11b k_compensate_bgr; the BGR compensation rule of include/bbme.h) at 4K on a colour
context after the cfg3 bidirectional estimate, beside the kernels that move comparable bytes:

  a1  K11b along the quarter-pel cells (unit 4), the frame        bbme_cells_compensate_bgr_device (d_out)
  a2  K11b unit 4, the statistics alone                           bbme_cells_compensate_bgr_device (d_stats4)
  a3  K11b unit 4, both from one launch
  b1  K11b along the integer cells (unit 1), the frame
  b2  K11b unit 1, the statistics alone
  b3  K11b unit 1, both from one launch
  c   K11 k_subpel_compensate on the luma planes, the frame       bbme_cells_subpel_compensate_device (d_out)
  d   K18b k_global_compensate_bgr on the same colour frames      bbme_cells_global_compensate_bgr_device (d_out)
  h1  on the host clock: bbme_compensation_error_bgr (unit 4: one refinement and one compensation launch, 32 bytes down) against
      downloading both stored colour frames and the quarter-pel grid and running bbme_compensate_bgr_host, alternating in one
      process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, the order swapping from run to run

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call.  Kernel times come from a separate run under rocprofv3:

    python scripts/compensation_bgr_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/compensation_bgr_probe.py --reps 100 --host-reps 0
    python scripts/compensation_bgr_probe.py --reps 100 --trace OUT      # the dispatches per case (no GPU needed)
    python scripts/compensation_bgr_probe.py --bench PARENT_CHECKOUT --bench-runs 3
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

from global_compensation_bgr_probe import _colour  # noqa: E402
from global_motion_probe import SIZE, TOL, WARMUP, _timed, bench  # noqa: E402

# (case, kernel, what)
CASES = [("a1", "k_compensate_bgr", "q4 frame"), ("a2", "k_compensate_bgr", "q4 stats"), ("a3", "k_compensate_bgr", "q4 both"),
         ("b1", "k_compensate_bgr", "int frame"), ("b2", "k_compensate_bgr", "int stats"), ("b3", "k_compensate_bgr", "int both"),
         ("c", "k_subpel_compensate", "luma"), ("d", "k_global_compensate_bgr", "frame")]


def run(reps, host_reps, device):
    import ctypes as C
    import numpy as np
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
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
    p1, p2 = mf.frame_plane_tensor(0, 0), mf.frame_plane_tensor(0, 1)
    c1, c2 = mf.frame_bgr_tensor(0, 0), mf.frame_bgr_tensor(0, 1)
    cells = mf.cells_tensor(0)
    q4 = torch.empty_like(cells)
    mf.cells_subpel_device(p1, p2, cells, out=q4)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    plane = torch.empty((H0, W0), dtype=torch.uint8, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    mf.synchronize()
    model = mf.global_motion(tol=TOL, window="all")["model"]
    print("4K colour: %dx%d (padded %dx%d, pads %d, %d), search %d, block %d, %d levels" % (w, h, W0, H0, mf.padding_x, mf.padding_y, search,
                                                                                           block, levels))
    print("%d calls per case after %d warm-up calls" % (reps, WARMUP))
    calls = {"a1": lambda: mf.cells_compensate_bgr_device(None, c2, q4, 4, out=out),
             "a2": lambda: mf.cells_compensate_bgr_device(c1, c2, q4, 4, stats=st),
             "a3": lambda: mf.cells_compensate_bgr_device(c1, c2, q4, 4, out=out, stats=st),
             "b1": lambda: mf.cells_compensate_bgr_device(None, c2, cells, 1, out=out),
             "b2": lambda: mf.cells_compensate_bgr_device(c1, c2, cells, 1, stats=st),
             "b3": lambda: mf.cells_compensate_bgr_device(c1, c2, cells, 1, out=out, stats=st),
             "c": lambda: mf.cells_compensate_subpel_device(None, p2, q4, out=plane),
             "d": lambda: mf.cells_global_compensate_bgr_device(None, c2, model, out=out)}
    for name, kernel, what in CASES:
        ev_ms, wall_ms = _timed(calls[name], reps, stream)
        print("  %-2s  %-24s %-9s: events %8.1f us, wall %8.1f us (medians)" % (name, kernel, what, ev_ms * 1e3, wall_ms * 1e3))
    if host_reps <= 0:                                      # a traced run: no dispatch behind the timed loops
        mf.close()
        return
    e1, e4, g4 = mf.compensation_error_bgr(), mf.compensation_error_subpel_bgr(), mf.compensation_error_subpel()
    print("  prediction of the unpadded frame: colour %.2f dB along the integer cells, %.2f dB along the quarter-pel cells (luma %.2f dB) "
          "over %d pixels (%d skipped)" % (e1["psnr"], e4["psnr"], g4["psnr"], e4["pixels"], e4["skipped"]))
    gpu, route, same = [], [], True
    for _ in range(host_reps):
        t0 = time.perf_counter()
        a = mf.compensation_error_subpel_bgr()
        gpu.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b = bbme.compensate_cells_bgr(c1.cpu().numpy(), c2.cpu().numpy(), mf.subpel_cells(), 4, 0, mf.padding_x, mf.padding_y)[1]
        route.append(time.perf_counter() - t0)
        same = same and a == b
    print("  h1 the residual of one pair on the host clock, medians of %d alternating calls: bbme_compensation_error_bgr %8.2f ms; "
          "both colour frames (%.1f MB) and the quarter-pel grid (%.1f MB) downloaded, then bbme_compensate_bgr_host %8.1f ms; equal: %s"
          % (host_reps, statistics.median(gpu) * 1e3, 2 * 3 * w * h / 1e6, W0 * H0 / 1e6, statistics.median(route) * 1e3, same))
    mf.close()


def report(trace_dir, reps):
    """Durations of each case's timed dispatches, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    print("kernel times from %s" % os.path.relpath(f, trace_dir))
    for kernel in ("k_compensate_bgr", "k_subpel_compensate", "k_global_compensate_bgr"):
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        cases = [c for c in CASES if c[1] == kernel]
        if len(dur) != len(cases) * (WARMUP + reps):
            raise SystemExit("%d %s dispatches, %d expected: not this probe's sequence (run it with --host-reps 0)"
                             % (len(dur), kernel, len(cases) * (WARMUP + reps)))
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
