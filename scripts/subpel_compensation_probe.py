"""Quarter-pel motion compensation (k_subpel_compensate, the subpel compensation rule of include/bbme.h) at 4K after the cfg3
estimate, beside k_motion_compensate on the same fields:

  a   the frame alone, along the refined cells                  bbme_cells_subpel_compensate_device (d_out)
  b   the statistics alone                                      bbme_cells_subpel_compensate_device (d_stats4)
  c   both from one launch                                      bbme_cells_subpel_compensate_device (d_out, d_stats4)
  d   k_motion_compensate, the frame alone (level 0, block 2)   bbme_motion_compensate_device
  e   k_motion_compensate, the statistics alone                 bbme_compensation_error (with its download and wait)
  h   per pair on the host: bbme_subpel_compensation_error against the route without this kernel -- download two planes and the
      quarter-pel cells, then bbme_subpel_compensate_host --, alternating in one process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, alternating, fresh processes

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call.  Kernel times come from a separate run under rocprofv3:

    python scripts/subpel_compensation_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/subpel_compensation_probe.py --reps 100 --host-reps 0
    python scripts/subpel_compensation_probe.py --reps 100 --trace OUT      # the dispatches per case (no GPU needed)
    python scripts/subpel_compensation_probe.py --bench PARENT_CHECKOUT --bench-runs 3
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

SIZE = (3840, 2160, 80, 16, 4)                             # bench.py's cfg3
WARMUP = 10
# (case, kernel, what)
CASES = [("a", "k_subpel_compensate", "frame"), ("b", "k_subpel_compensate", "stats"), ("c", "k_subpel_compensate", "both"),
         ("d", "k_motion_compensate", "frame"), ("e", "k_motion_compensate", "stats")]


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


def run(reps, host_reps, device):
    import ctypes as C
    import numpy as np
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    w, h, search, block, levels = SIZE
    f1, f2, _ = bbme.synth_pair(w, h, 1030, max_motion=24)
    mf = bbme.MF(f1, f2, [search] * levels, [block] * levels, levels, device=device)
    mf.estimate_async()
    mf.synchronize()
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    dev = "cuda:%d" % device
    ch, cw = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    p1, p2 = (torch.from_numpy(p).to(dev) for p in mf.get_level_planes(0))
    q4 = torch.empty((ch, cw, 2), dtype=torch.int16, device=dev)
    _capi.check(mf._lib.bbme_subpel_device(mf._ctx, 0, 0, C.c_void_p(q4.data_ptr()), cw, None))
    out = torch.empty((H0, W0), dtype=torch.uint8, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    mf.synchronize()
    print("4K: %dx%d (padded %dx%d), search %d, block %d, %d levels: %d cells" % (w, h, W0, H0, search, block, levels, ch * cw))
    print("%d calls per case after %d warm-up calls" % (reps, WARMUP))
    calls = {("k_subpel_compensate", "frame"): lambda: mf.cells_compensate_subpel_device(None, p2, q4, out=out),
             ("k_subpel_compensate", "stats"): lambda: mf.cells_compensate_subpel_device(p1, p2, q4, stats=st),
             ("k_subpel_compensate", "both"): lambda: mf.cells_compensate_subpel_device(p1, p2, q4, out=out, stats=st),
             ("k_motion_compensate", "frame"): lambda: mf.motion_compensated_device(out),
             ("k_motion_compensate", "stats"): lambda: mf.compensation_error(0, 2)}
    for name, kernel, what in CASES:
        ev_ms, wall_ms = _timed(calls[(kernel, what)], reps, stream)
        print("  %s  %-19s %-5s: events %8.1f us, wall %8.1f us (medians)" % (name, kernel, what, ev_ms * 1e3, wall_ms * 1e3))
    e_int, e_q4 = mf.compensation_error(0, 2), mf.compensation_error_subpel()
    print("  prediction of the unpadded frame: integer cells %.2f dB, quarter-pel cells %.2f dB" % (e_int["psnr"], e_q4["psnr"]))
    gpu, route, same = [], [], True
    for _ in range(host_reps):
        t0 = time.perf_counter()
        a = mf.compensation_error_subpel()
        gpu.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h1, h2 = mf.get_level_planes(0)
        _, b = bbme.compensate_cells_subpel(h1, h2, mf.subpel_cells(), 0,
                                            (mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height))
        route.append(time.perf_counter() - t0)
        same = same and a == b
    if host_reps > 0:
        print("  h  one pair's statistics on the host, medians of %d alternating calls: bbme_subpel_compensation_error %8.2f ms; two "
              "planes and the quarter-pel cells downloaded, then bbme_subpel_compensate_host %8.1f ms; equal: %s"
              % (host_reps, statistics.median(gpu) * 1e3, statistics.median(route) * 1e3, same))
    mf.close()


def report(trace_dir, reps):
    """Durations of each case's timed dispatches, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    print("kernel times from %s" % os.path.relpath(f, trace_dir))
    for kernel in ("k_subpel_compensate", "k_motion_compensate"):
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        cases = [c for c in CASES if c[1] == kernel]
        expected = len(cases) * (WARMUP + reps) + 1                         # + the PSNR line's call behind the timed loops
        if len(dur) != expected:
            raise SystemExit("%d %s dispatches, %d expected: not this probe's sequence (run it with --host-reps 0)"
                             % (len(dur), kernel, expected))
        for k, (name, _, what) in enumerate(cases):
            timed = dur[k * (WARMUP + reps) + WARMUP:(k + 1) * (WARMUP + reps)]
            print("  %s  %-19s %-5s: kernel %7.1f us median (min %.1f, max %.1f) of %d" % (name, kernel, what, statistics.median(timed),
                                                                                          min(timed), max(timed), len(timed)))


def bench(parent, runs, steps, warmup):
    """bench.py of this tree and of the parent's checkout, alternating, a fresh process each: every `value` and the medians"""
    values = {"this": [], "parent": []}
    for _ in range(runs):
        for name, root in (("parent", parent), ("this", ROOT)):
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
