"""Global motion and global compensation (K16 k_vector_histogram, K17 k_global_moments, K18 k_global_compensate; the global motion
rule and the global compensation rule of include/bbme.h) at 4K after the cfg3 bidirectional estimate, beside the kernels that move
the same bytes:

  a1  K16 on the estimated forward cells                         bbme_cells_vector_histogram_device
  a2  K16 on a uniform grid (one add per wave and component)
  a3  K16 on a random grid (up to 64 turns of the aggregation loop per wave and component)
  b1  K17, the sixteen words alone                               bbme_cells_global_moments_device (d_words16)
  b2  K17, map and words                                         bbme_cells_global_moments_device (d_map, d_words16)
  c1  K18, the frame alone                                       bbme_cells_global_compensate_device (d_out)
  c2  K18, the statistics alone                                  bbme_cells_global_compensate_device (d_stats4)
  c3  K18, both from one launch
  d   k_fb_consistency, mask and statistics (K16's and K17's grid bytes)      bbme_cells_consistency_device
  e   k_subpel_compensate, the frame alone (K18's plane bytes)                bbme_cells_subpel_compensate_device
  h   the whole estimate on the host clock: bbme_global_motion (affine, 3 iterations, every pair, a step's wait each) against
      downloading the cells and running bbme_global_motion_host, alternating in one process
  B   bench.py's `value` of this build and of a built checkout of the parent commit, the order swapping from run to run

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call.  Kernel times come from a separate run under rocprofv3:

    python scripts/global_motion_probe.py --reps 100
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/global_motion_probe.py --reps 100 --host-reps 0
    python scripts/global_motion_probe.py --reps 100 --trace OUT      # the dispatches per case (no GPU needed)
    python scripts/global_motion_probe.py --bench PARENT_CHECKOUT --bench-runs 3
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
TOL = 64                                                   # pixels
# (case, kernel, what)
CASES = [("a1", "k_vector_histogram", "estimated"), ("a2", "k_vector_histogram", "uniform"), ("a3", "k_vector_histogram", "random"),
         ("b1", "k_global_moments", "words"), ("b2", "k_global_moments", "map+words"),
         ("c1", "k_global_compensate", "frame"), ("c2", "k_global_compensate", "stats"), ("c3", "k_global_compensate", "both"),
         ("d", "k_fb_consistency", "mask+stats"), ("e", "k_subpel_compensate", "frame")]


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
    mf.estimate_bidirectional_async()
    mf.synchronize()
    handle = C.c_void_p()
    _capi.check(mf._lib.bbme_get_stream(mf._ctx, C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value)
    dev = "cuda:%d" % device
    ch, cw = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    p1, p2 = (torch.from_numpy(p).to(dev) for p in mf.get_level_planes(0))
    fwd, bwd = mf.cells_tensor(0), mf.backward_cells_tensor(0)
    uniform = torch.empty((ch, cw, 2), dtype=torch.int16, device=dev)
    uniform[..., 0], uniform[..., 1] = 3, -2
    rnd = torch.from_numpy(np.random.default_rng(7).integers(-1024, 1024, size=(ch, cw, 2)).astype(np.int16)).to(dev)
    q4 = torch.empty((ch, cw, 2), dtype=torch.int16, device=dev)
    _capi.check(mf._lib.bbme_subpel_device(mf._ctx, 0, 0, C.c_void_p(q4.data_ptr()), cw, None))
    hist = torch.empty((2, 2048), dtype=torch.int32, device=dev)
    words = torch.zeros(16, dtype=torch.int64, device=dev)
    gmap = torch.empty((ch, cw), dtype=torch.uint8, device=dev)
    mask = torch.empty((ch, cw), dtype=torch.uint8, device=dev)
    out = torch.empty((H0, W0), dtype=torch.uint8, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    mf.synchronize()
    # the pair is 4 x 4 tiles of independent motions: no vector is dominant, so the tolerance is TOL pixels, at which every cell is
    # an inlier of the fitted model and K17 adds up all its sums
    got = mf.global_motion(tol=TOL, window="all")
    model = got["model"]
    print("4K: %dx%d (padded %dx%d), search %d, block %d, %d levels: %d cells" % (w, h, W0, H0, search, block, levels, ch * cw))
    print("model of the estimated field (affine, tol %d px, 3 iterations, all cells): %s, inliers %d outliers %d"
          % (TOL, model.tolist(), got["statistics"]["inliers"], got["statistics"]["outliers"]))
    print("%d calls per case after %d warm-up calls" % (reps, WARMUP))
    calls = {"a1": lambda: mf.cells_vector_histogram_device(fwd, hist),
             "a2": lambda: mf.cells_vector_histogram_device(uniform, hist),
             "a3": lambda: mf.cells_vector_histogram_device(rnd, hist),
             "b1": lambda: mf.cells_global_moments_device(fwd, model, TOL * 65536, words=words),
             "b2": lambda: mf.cells_global_moments_device(fwd, model, TOL * 65536, map=gmap, words=words),
             "c1": lambda: mf.cells_global_compensate_device(None, p2, model, out=out),
             "c2": lambda: mf.cells_global_compensate_device(p1, p2, model, stats=st),
             "c3": lambda: mf.cells_global_compensate_device(p1, p2, model, out=out, stats=st),
             "d": lambda: mf.cells_consistency_device(fwd, bwd, 1, mask=mask, stats=st),
             "e": lambda: mf.cells_compensate_subpel_device(None, p2, q4, out=out)}
    for name, kernel, what in CASES:
        ev_ms, wall_ms = _timed(calls[name], reps, stream)
        print("  %-2s  %-19s %-9s: events %8.1f us, wall %8.1f us (medians)" % (name, kernel, what, ev_ms * 1e3, wall_ms * 1e3))
    e_blk, e_glb = mf.compensation_error(0, 2), mf.compensation_error_global(model)
    print("  prediction of the unpadded frame: block field %.2f dB, global model %.2f dB" % (e_blk["psnr"], e_glb["psnr"]))
    gpu, route, same = [], [], True
    for _ in range(host_reps):
        t0 = time.perf_counter()
        a = mf._global_motion("forward", False, "affine", TOL, 3, None, "all")[0]
        gpu.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        m, wds, _ = bbme.global_motion_cells(mf.get_cells(), "affine", TOL * 65536, 3)
        route.append(time.perf_counter() - t0)
        same = same and np.array_equal(a["model"], m) and list(a["statistics"].values()) == wds.tolist()
    if host_reps > 0:
        print("  h  one pair's estimate on the host clock, medians of %d alternating calls: bbme_global_motion %8.2f ms; the cells "
              "downloaded (%.1f MB), then bbme_global_motion_host %8.1f ms; equal: %s"
              % (host_reps, statistics.median(gpu) * 1e3, ch * cw * 4 / 1e6, statistics.median(route) * 1e3, same))
    mf.close()


def report(trace_dir, reps):
    """Durations of each case's timed dispatches, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    print("kernel times from %s" % os.path.relpath(f, trace_dir))
    # dispatches of each kernel in front of the timed loops: the model's estimate (one K16; up to three K17 passes, the last one and
    # the map's), and behind them: the PSNR line's K18
    lead = {"k_vector_histogram": (1, 1), "k_global_moments": (2, 5), "k_global_compensate": (0, 0), "k_fb_consistency": (0, 0),
            "k_subpel_compensate": (0, 0)}
    tail = {"k_global_compensate": 1}
    for kernel in lead:
        dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        cases = [c for c in CASES if c[1] == kernel]
        first = len(dur) - len(cases) * (WARMUP + reps) - tail.get(kernel, 0)
        if not lead[kernel][0] <= first <= lead[kernel][1]:
            raise SystemExit("%d %s dispatches, %d + %d .. %d expected: not this probe's sequence (run it with --host-reps 0)"
                             % (len(dur), kernel, len(cases) * (WARMUP + reps) + tail.get(kernel, 0), lead[kernel][0], lead[kernel][1]))
        dur = dur[first:]
        for k, (name, _, what) in enumerate(cases):
            timed = dur[k * (WARMUP + reps) + WARMUP:(k + 1) * (WARMUP + reps)]
            print("  %-2s  %-19s %-9s: kernel %7.1f us median (min %.1f, max %.1f) of %d" % (name, kernel, what, statistics.median(timed),
                                                                                             min(timed), max(timed), len(timed)))
    red = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "k_reduce_words" in r["Kernel_Name"]]
    if red:
        print("      k_reduce_words (behind every K17 launch with words): kernel %7.1f us median of %d" % (statistics.median(red), len(red)))


def bench(parent, runs, steps, warmup):
    """bench.py of this tree and of the parent's checkout, a fresh process each, the order swapping from run to run"""
    values = {"this": [], "parent": []}
    order = [("parent", parent), ("this", ROOT)]
    for k in range(runs):
        for name, root in (order if k % 2 == 0 else order[::-1]):
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=root, capture_output=True, text=True, check=True, timeout=300)
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
