"""Colour coding of the motion field on the GPU (k_color_range, k_color_image; the colour rule of include/bbme.h) at the sizes a
user runs:

  a   cfg3 4K estimate, scale 1: range pass + image        bbme_flow_color_device
  b   the reference's literals (4 levels, block 32, search 64) on 960x540 frames up-sampled x4, scale 4: range pass + image
  c   6 cfg3 pairs (2 distinct, each 3 times): the ranges of all pairs in one launch     bbme_flow_ranges
  w   per picture on the host: the device route (MF.flow_color: image and range made on the GPU, 3 B/pixel downloaded) and the
      host route it replaces (MF.get_subsampled_flow: 8 B/pixel downloaded, then Flow.MotionToColor on one core), alternating

Per GPU case: the median over --reps calls after warm-up of the time between two HIP events on the context's stream around the
call, and of the host wall time of the call; the bytes the kernels must move, computed from the shapes (4 B per sampled cell
read by each pass, 3 B per pixel written), and what those bytes take at the 3.8 TB/s k_fb_consistency reached
(profiles/r08_bidirectional.txt).  Kernel times come from a separate run under rocprofv3:

    python scripts/flow_color_probe.py --reps 100
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/flow_color_probe.py --reps 100 --host-reps 0
    python scripts/flow_color_probe.py --reps 100 --trace OUT      # the two kernels' dispatches per case (no GPU needed)
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
REF_SEARCH, REF_BLOCK, REF_LEVELS = 64, 32, 4              # main_class.cpp:19-21
REF_W, REF_H = 960, 540                                    # up-sampled x4: 3840 x 2160
REACHED_GBS = 3800.0                                       # k_fb_consistency, profiles/r08_bidirectional.txt
WARMUP = 10
BATCH, DISTINCT = 6, 2
# name, what, width, height, scale, pairs, image written
CASES = [("a", "cfg3, scale 1", W, H, 1, 1, True), ("b", "reference x4, scale 4", 4 * REF_W, 4 * REF_H, 4, 1, True),
         ("c", "ranges x6, scale 1", W, H, 1, BATCH, False)]


def sampled_cells(w, h, pad_x, pad_y, scale):
    if scale == 1:
        return (((pad_x + w - 1) >> 1) - (pad_x >> 1) + 1) * (((pad_y + h - 1) >> 1) - (pad_y >> 1) + 1)
    return -(-w // scale) * -(-h // scale)


def kernel_bytes(w, h, pad_x, pad_y, scale, pairs, image):
    """(range pass, image pass): 4 B per sampled cell read by each, 3 B per pixel written by the second."""
    cells = sampled_cells(w, h, pad_x, pad_y, scale)
    return pairs * 4 * cells, (4 * cells + 3 * -(-w // scale) * -(-h // scale)) if image else 0


def pads(w, h, search, block, levels):
    from blockbasedmotionestimation_amd.motion_framework import plan_padding
    return plan_padding(w, h, [search] * levels, [block] * levels)[2:]


def run(reps, host_reps, device):
    import ctypes as C
    import torch
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    ss, bs = [SEARCH] * LEVELS, [BLOCK] * LEVELS
    pairs = [bbme.synth_pair(W, H, 1000 + 30 + k, max_motion=24)[:2] for k in range(DISTINCT)]
    mf = bbme.MF(pairs[0][0], pairs[0][1], ss, bs, LEVELS, device=device)
    mf.estimate_async()
    small = bbme.synth_pair(REF_W, REF_H, 1040, max_motion=6)[:2]
    mr = bbme.MF(small[0], small[1], [REF_SEARCH] * REF_LEVELS, [REF_BLOCK] * REF_LEVELS, REF_LEVELS, device=device, upsample=4)
    mr.estimate_async()
    mb = bbme.MFBatch([pairs[k % DISTINCT] for k in range(BATCH)], ss, bs, LEVELS, device=device)
    mb.estimate_async()
    for m in (mf, mr, mb):
        m.synchronize()

    def ctx_stream(m):
        handle = C.c_void_p()
        _capi.check(m._lib.bbme_get_stream(m._ctx, C.byref(handle)))
        return torch.cuda.ExternalStream(handle.value)

    rng = torch.empty(5, dtype=torch.float32, device="cuda:%d" % device)
    out_a = torch.empty(mf.color_shape(1), dtype=torch.uint8, device="cuda:%d" % device)
    out_b = torch.empty(mr.color_shape(4), dtype=torch.uint8, device="cuda:%d" % device)
    calls = {
        "a": (mf, ctx_stream(mf), lambda: mf.flow_color_device(out_a, 1, range=rng)),
        "b": (mr, ctx_stream(mr), lambda: mr.flow_color_device(out_b, 4, range=rng)),
        "c": (mb, ctx_stream(mb), lambda: mb.flow_ranges_all("forward", 1)),
    }
    print("colour coding after bbme_estimate; %d calls per case after %d warm-up calls; bytes: 4 B per sampled cell read by each pass, "
          "3 B per pixel written; 'at 3.8 TB/s' = what those bytes take at the rate k_fb_consistency reached" % (reps, WARMUP))
    for name, what, w, h, scale, npairs, image in CASES:
        m, st, fn = calls[name]
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
        rb, ib = kernel_bytes(w, h, m.padding_x, m.padding_y, scale, npairs, image)
        print("  %s  %-22s: events %8.1f us, wall %8.1f us (medians); range pass %6.2f MB, image pass %6.2f MB -> %5.1f us at 3.8 TB/s"
              % (name, what, ev_ms * 1e3, statistics.median(wall) * 1e6, rb / 1e6, ib / 1e6, (rb + ib) / REACHED_GBS / 1e3))
    print("  ranges: a %s  b %s" % (mf.flow_range("forward", 1), mr.flow_range("forward", 4)))
    print("  pair 0 of the batch equals the single context: %s"
          % (tuple(float(v) for v in mb.flow_ranges_all("forward", 1)[0]) == mf.flow_range("forward", 1),))
    if host_reps > 0:
        flow = bbme.Flow()
        for name, m, scale in (("a", mf, 1), ("b", mr, 4)):
            dev, host = [], []
            for _ in range(host_reps):
                t0 = time.perf_counter()
                img = m.flow_color(scale)
                t1 = time.perf_counter()
                field = m.get_subsampled_flow(scale)
                ref = flow.MotionToColor(field, verbose=False)
                t2 = time.perf_counter()
                dev.append(t1 - t0)
                host.append(t2 - t1)
            d = (img != ref)
            print("  w  %s, scale %d, %dx%d picture: device route %8.2f ms (%.1f MB over PCIe), host route %8.2f ms (%.1f MB over PCIe) per picture, "
                  "medians of %d, alternating" % (name, scale, img.shape[1], img.shape[0], statistics.median(dev) * 1e3, img.nbytes / 1e6,
                                                  statistics.median(host) * 1e3, field.nbytes / 1e6, host_reps))
            print("     ranges equal: %s; channels that differ between the routes (the angle decision of include/bbme.h): %d of %d, "
                  "none by more than %d" % (m.last_color_range == flow.last_range, int(d.sum()), d.size,
                                            int(abs(img.astype(int) - ref.astype(int)).max())))
    for m in (mb, mr, mf):
        m.close()


def report(trace_dir, reps):
    """Durations of the k_color_range / k_color_image dispatches of each case's timed calls, in the order the probe issues them."""
    f = max(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}
    for r in rows:
        dur.setdefault(r["Kernel_Name"].split("(")[0].split("::")[-1].replace(".kd", "").strip(), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    per_case = WARMUP + reps
    expected = {"k_color_range": 3 * per_case + 4, "k_color_image": 2 * per_case}     # + the four range calls after the timed loops
    for k, n in expected.items():
        got = len(dur.get(k, []))
        print("kernel times from %s: %d %s dispatches (%d expected)" % (os.path.relpath(f, trace_dir), got, k, n))
        if got != n:
            raise SystemExit("the trace does not hold the probe's dispatch sequence (run it with --host-reps 0)")
    for k, (name, what, w, h, scale, npairs, image) in enumerate(CASES):
        if name == "b":
            px, py = pads(w, h, REF_SEARCH, REF_BLOCK, REF_LEVELS)
        else:
            px, py = pads(w, h, SEARCH, BLOCK, LEVELS)
        rb, ib = kernel_bytes(w, h, px, py, scale, npairs, image)
        for kern, nb in (("k_color_range", rb), ("k_color_image", ib)):
            if not nb:
                continue
            timed = dur[kern][k * per_case + WARMUP:(k + 1) * per_case]
            t = statistics.median(timed)
            print("  %s  %-22s %-14s: kernel %7.1f us median (min %.1f, max %.1f); %6.2f MB = %5.1f us at 3.8 TB/s (x%.1f)"
                  % (name, what, kern, t, min(timed), max(timed), nb / 1e6, nb / REACHED_GBS / 1e3, t / (nb / REACHED_GBS / 1e3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--trace", help="report the kernel times of a rocprofv3 --kernel-trace run of this probe")
    args = ap.parse_args()
    if args.trace:
        report(args.trace, args.reps)
    else:
        run(args.reps, args.host_reps, args.device)


if __name__ == "__main__":
    main()
