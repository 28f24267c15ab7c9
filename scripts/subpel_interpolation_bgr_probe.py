"""Colour interpolation at quarter-pel positions (K12b k_subpel_interpolate_bgr, the BGR subpel interpolation rule of
include/bbme.h) at 4K after the cfg3 bidirectional estimate on colour frames, beside k_interpolate_bgr and k_subpel_interpolate
on the same fields in the same run:

  a   one colour frame, phase 1 / 2, along the refined fields      bbme_cells_subpel_interpolate_bgr_device (stored colour)
  b   a run of three colour frames, phases 1 / 4 .. 3 / 4          bbme_cells_subpel_interpolate_bgr_device (count 3)
  c   k_interpolate_bgr, one frame along the integer fields        bbme_cells_interpolate_bgr_device
  d   k_interpolate_bgr, a run of three frames                     bbme_cells_interpolate_bgr_device (count 3)
  e   k_subpel_interpolate, one grey frame along the refined fields    bbme_cells_subpel_interpolate_device (d_out)
  f   k_subpel_interpolate, a run of three grey frames             bbme_cells_subpel_interpolate_device (d_out, count 3)
  r   the two k_subpel_refine launches that make the quarter-pel grids (forward, then backward)    bbme_subpel_device
  h   per pair on the host: bbme_get_subpel_interpolated_bgr_host against the route without this kernel -- download both planes,
      both quarter-pel grids and both colour frames, then bbme_subpel_interpolate_bgr_host --, alternating in one process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, alternating (the order of the two swaps
      from run to run: parent, this, this, parent, ...), fresh processes

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call.  Kernel times come from a separate run under rocprofv3:

    python scripts/subpel_interpolation_bgr_probe.py --reps 100
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/subpel_interpolation_bgr_probe.py --reps 100 --host-reps 0
    python scripts/subpel_interpolation_bgr_probe.py --reps 100 --trace OUT      # the dispatches per case (no GPU needed)
    python scripts/subpel_interpolation_bgr_probe.py --bench PARENT_CHECKOUT --bench-runs 3
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from subpel_interpolation_probe import SIZE, WARMUP, _timed  # noqa: E402

# (case, kernel, what)
CASES = [("a", "k_subpel_interpolate_bgr", "frame"), ("b", "k_subpel_interpolate_bgr", "run3"), ("c", "k_interpolate_bgr", "frame"),
         ("d", "k_interpolate_bgr", "run3"), ("e", "k_subpel_interpolate", "frame"), ("f", "k_subpel_interpolate", "run3"),
         ("r", "k_subpel_refine", "both")]


def run(reps, host_reps, device):
    import ctypes as C
    import numpy as np
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    w, h, search, block, levels = SIZE
    g1, g2, _ = bbme.synth_pair(w, h, 1030, max_motion=24)
    c1, c2 = (np.ascontiguousarray(np.stack([g, 255 - g, (g.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1)) for g in (g1, g2))
    mf = bbme.MF(c1, c2, [search] * levels, [block] * levels, levels, device=device)
    mf.estimate_bidirectional_async()
    mf.synchronize()
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    dev = "cuda:%d" % device
    ch, cw = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    fwd, bwd = (torch.from_numpy(g).to(dev) for g in (mf.get_cells(), mf.get_backward_cells()))
    t1, t2 = torch.from_numpy(c1).to(dev), torch.from_numpy(c2).to(dev)
    q4 = torch.empty((2, ch, cw, 2), dtype=torch.int16, device=dev)

    def refine():
        for which in (0, 1):
            _capi.check(mf._lib.bbme_subpel_device(mf._ctx, 0, which, C.c_void_p(q4[which].data_ptr()), cw, None))

    refine()
    out = torch.empty((3, h, w, 3), dtype=torch.uint8, device=dev)
    grey = torch.empty((3, H0, W0), dtype=torch.uint8, device=dev)
    mf.synchronize()
    print("4K colour: %dx%d (padded %dx%d, padding %d, %d), search %d, block %d, %d levels: %d cells"
          % (w, h, W0, H0, mf.padding_x, mf.padding_y, search, block, levels, ch * cw))
    print("%d calls per case after %d warm-up calls" % (reps, WARMUP))
    calls = {("k_subpel_interpolate_bgr", "frame"): lambda: mf.cells_interpolate_subpel_bgr_device(q4[0], q4[1], None, None, 1, 1, 2, out=out[:1]),
             ("k_subpel_interpolate_bgr", "run3"): lambda: mf.cells_interpolate_subpel_bgr_device(q4[0], q4[1], None, None, 1, 3, 4, out=out),
             ("k_interpolate_bgr", "frame"): lambda: mf.cells_interpolate_bgr_device(fwd, bwd, None, None, 1, 1, 2, out=out[:1]),
             ("k_interpolate_bgr", "run3"): lambda: mf.cells_interpolate_bgr_device(fwd, bwd, None, None, 1, 3, 4, out=out),
             ("k_subpel_interpolate", "frame"): lambda: mf.cells_interpolate_subpel_device(q4[0], q4[1], 1, 1, 2, out=grey[:1]),
             ("k_subpel_interpolate", "run3"): lambda: mf.cells_interpolate_subpel_device(q4[0], q4[1], 1, 3, 4, out=grey),
             ("k_subpel_refine", "both"): refine}
    for name, kernel, what in CASES:
        ev_ms, wall_ms = _timed(calls[(kernel, what)], reps, stream)
        print("  %s  %-24s %-5s: events %8.1f us, wall %8.1f us (medians)" % (name, kernel, what, ev_ms * 1e3, wall_ms * 1e3))
    gpu, route, same = [], [], True
    for _ in range(host_reps):
        t0 = time.perf_counter()
        a = mf.interpolate_subpel_bgr(1, 2)
        gpu.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        h1, h2 = mf.get_level_planes(0)
        d1, d2 = t1.cpu().numpy(), t2.cpu().numpy()           # the colour frames' bytes, as the stored colour would come down
        b = bbme.interpolate_cells_subpel_bgr(h1, h2, d1, d2, mf.subpel_cells("forward"), mf.subpel_cells("backward"), 1, 2,
                                              mf.padding_x, mf.padding_y)
        route.append(time.perf_counter() - t0)
        same = same and np.array_equal(a, b)
    if host_reps > 0:
        print("  h  one pair's colour frame on the host, medians of %d alternating calls: bbme_get_subpel_interpolated_bgr_host %8.2f ms; "
              "both planes, both quarter-pel grids and both colour frames downloaded, then bbme_subpel_interpolate_bgr_host %8.1f ms; "
              "equal: %s" % (host_reps, statistics.median(gpu) * 1e3, statistics.median(route) * 1e3, same))
    mf.close()


def report(trace_dir, reps):
    """Durations of each case's timed dispatches, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    print("kernel times from %s" % os.path.relpath(f, trace_dir))

    def durations(kernel):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
                if kernel in r["Kernel_Name"] and kernel + "_" not in r["Kernel_Name"]]

    def line(name, kernel, what, timed):
        print("  %s  %-24s %-8s: kernel %7.1f us median (min %.1f, max %.1f) of %d" % (name, kernel, what, statistics.median(timed),
                                                                                        min(timed), max(timed), len(timed)))

    for kernel in ("k_subpel_interpolate_bgr", "k_interpolate_bgr", "k_subpel_interpolate"):
        dur = durations(kernel)
        cases = [c for c in CASES if c[1] == kernel]
        expected = len(cases) * (WARMUP + reps)
        if len(dur) != expected:
            raise SystemExit("%d %s dispatches, %d expected: not this probe's sequence (run it with --host-reps 0)"
                             % (len(dur), kernel, expected))
        for k, (name, _, what) in enumerate(cases):
            line(name, kernel, what, dur[k * (WARMUP + reps) + WARMUP:(k + 1) * (WARMUP + reps)])
    # k_subpel_refine: the two launches that fill q4, then the timed case's pairs (forward, backward)
    dur = durations("k_subpel_refine")
    if len(dur) != 2 + 2 * (WARMUP + reps):
        raise SystemExit("%d k_subpel_refine dispatches, %d expected: not this probe's sequence (run it with --host-reps 0)"
                         % (len(dur), 2 + 2 * (WARMUP + reps)))
    timed = dur[2 + 2 * WARMUP:]
    line("r", "k_subpel_refine", "forward", timed[0::2])
    line("r", "k_subpel_refine", "backward", timed[1::2])


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
