"""Both fields (frame p -> p + 1 and p + 1 -> p) of the consecutive pairs of a video two ways, on the same seeded video and
the same shape of contexts:

  (a) two-pass  what a caller without bbme_estimate_bidirectional does: the forward fields on chain contexts (MFChain: every
                frame set once), plus the exchanged pairs (f_p+1, f_p) on batched contexts (MFBatch) fed pair by pair -- both
                frames of every pair uploaded, padded and pyramided a second time
  (b) one-pass  estimate_bidirectional_async on chain contexts alone: every frame set once, both estimates from those planes

A round = set the frames of every context, enqueue its estimate(s), then download both cell grids of every pair into pinned
memory.  Wall milliseconds per pair on the host clock around that synchronised work, (a) and (b) alternating round by round in
one process after 3 warm-up rounds, pinned host frames, each measurement made twice to show the spread; the bytes each form
uploads (from the shapes); an assertion that all fields of (a) equal (b)'s, with a CRC.

  python scripts/bidirectional_pipeline.py [--rounds 20] [--shapes 4k_4x2,4k_4x6,1080p_4x8]
  python scripts/bidirectional_pipeline.py --direction          # estimate_async in direction BACKWARD against FORWARD
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bidirectional_pipeline.py --kernel [--reps 20]
  python scripts/bidirectional_pipeline.py --report DIR [--reps 20]     # k_fb_consistency's times from that trace

--kernel: no timing of its own; at 4K, after one bidirectional estimate of a chain of six pairs, `--reps` launches each of
k_fb_consistency for one pair with the mask only, the statistics only and both, and for all six pairs (statistics; the mask
calls address one pair), then as many of k_motion_compensate's frame-only pass.  --report groups the trace's dispatches in
that order.
"""
import argparse
import csv
import ctypes as C
import glob
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import blockbasedmotionestimation_amd as bbme  # noqa: E402
from blockbasedmotionestimation_amd import _capi  # noqa: E402
from video_pipeline import POOL, SHAPES, Video, median_min, pinned_like  # noqa: E402

KERNEL_VARIANTS = ("1 pair, mask only", "1 pair, statistics only", "1 pair, mask + statistics", "6 pairs, statistics only")


class Forms:
    """The two forms over `contexts` contexts of `pairs` pairs; context c starts at frame c * stride of the video."""

    def __init__(self, shape, video, device, stride):
        w, h, search, block, levels, self.contexts, self.pairs = shape
        self.w, self.video, self.stride = w, video, stride
        ss, bs = [search] * levels, [block] * levels
        first = [[video[c * stride + i] for i in range(self.pairs + 1)] for c in range(self.contexts)]
        self.forward = [bbme.MFChain(f, ss, bs, levels, device=device) for f in first]
        self.exchanged = [bbme.MFBatch([(b, a) for a, b in zip(f, f[1:])], ss, bs, levels, device=device) for f in first]
        self.both = [bbme.MFChain(f, ss, bs, levels, device=device) for f in first]
        for mf in self.forward + self.exchanged + self.both:
            mf.set_speculation(False)                  # several pairs in flight fill the chip already
        shape_c = (self.both[0].padded_height // 2, self.both[0].padded_width // 2, 2)
        import torch
        self._keep = [torch.empty((2, self.contexts, self.pairs) + shape_c, dtype=torch.int16).pin_memory() for _ in range(2)]
        self.cells = [t.numpy() for t in self._keep]   # [form][direction, context, pair]

    def close(self):
        for mf in self.forward + self.exchanged + self.both:
            mf.close()

    def frames_of_round(self, c, r):
        k = c * self.stride + r * self.pairs
        return [self.video[k + i] for i in range(self.pairs + 1)]

    def round_two_pass(self, r):
        lib = _capi.lib()
        for c in range(self.contexts):
            f = self.frames_of_round(c, r)
            self.forward[c].advance(f[1:], wait=False)
            self.forward[c].estimate_async()
            mb = self.exchanged[c]
            for p in range(self.pairs):
                _capi.check(lib.bbme_set_frames_host_async(mb._ctx, p, f[p + 1].ctypes.data, f[p].ctypes.data, self.w))
            mb.estimate_async()
        for c in range(self.contexts):
            for p in range(self.pairs):
                self.forward[c].get_pair_cells(p, out=self.cells[0][0, c, p])
                self.exchanged[c].get_pair_cells(p, out=self.cells[0][1, c, p])

    def round_one_pass(self, r):
        for c, mf in enumerate(self.both):
            mf.advance(self.frames_of_round(c, r)[1:], wait=False)
            mf.estimate_bidirectional_async()
        for c, mf in enumerate(self.both):
            for p in range(self.pairs):
                mf.get_pair_cells(p, out=self.cells[1][0, c, p])
                mf.get_pair_backward_cells(p, out=self.cells[1][1, c, p])

    def check_round(self, r, what):
        if not np.array_equal(self.cells[0], self.cells[1]):
            bad = [(d, c, p) for d in range(2) for c in range(self.contexts) for p in range(self.pairs)
                   if not np.array_equal(self.cells[0][d, c, p], self.cells[1][d, c, p])]
            raise AssertionError("%s, round %d: the fields of (a) and (b) differ for (direction, context, pair) %s" % (what, r, bad))
        if np.array_equal(self.cells[0][0], self.cells[0][1]):
            raise AssertionError("%s, round %d: forward and backward fields are the same" % (what, r))
        return zlib.crc32(self.cells[0].tobytes())


def timed_rounds(forms, first_round, rounds, what):
    ta, tb, crc = [], [], 0
    for r in range(first_round, first_round + rounds):
        t0 = time.perf_counter()
        forms.round_two_pass(r)
        t1 = time.perf_counter()
        forms.round_one_pass(r)
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
        crc ^= forms.check_round(r, what)              # outside both timers
    n = forms.contexts * forms.pairs
    return [x / n for x in ta], [x / n for x in tb], crc


def run_shape(name, shape, rounds, device):
    w, h, search, block, levels, contexts, pairs = shape
    pool = bbme.synth_video(w, h, POOL, 4242, max_motion=8)
    pinned, keep = pinned_like(pool)
    print("%s: %dx%d, search %d, block %d, %d levels; %d contexts x %d pairs = %d pairs per round; %d timed rounds per figure" %
          (name, w, h, search, block, levels, contexts, pairs, contexts * pairs, rounds))
    print("  upload per pair (from the shapes): (a) %d B = W H for the chain + 2 W H for the exchanged pair;  (b) %d B = W H" %
          (3 * w * h, w * h))
    forms = Forms(shape, Video(pinned), device, 2 * pairs + 1)
    CH, CW = forms.both[0].cells_shape
    print("  download per pair, both forms: %d B = 2 grids of 4 B x %d x %d cells of the padded plane" % (8 * CH * CW, CW, CH))
    nxt = 1
    for r in range(nxt, nxt + 3):                      # warm-up: graphs captured, buffers allocated
        forms.round_two_pass(r)
        forms.round_one_pass(r)
        forms.check_round(r, name)
    nxt += 3
    for rep in range(2):
        ta, tb, crc = timed_rounds(forms, nxt, rounds, name)
        nxt += rounds
        (ma, mina), (mb, minb) = median_min(ta), median_min(tb)
        print("  run %d: (a) two-pass %7.3f ms/pair median (min %.3f)   (b) one-pass %7.3f ms/pair median (min %.3f)   (a)/(b) %.2f   "
              "fields equal: yes (crc %08x)" % (rep + 1, ma, mina, mb, minb, ma / mb, crc))
        sys.stdout.flush()
    forms.close()
    del keep


def run_direction(device, reps, backward_first=False):
    """estimate_async + synchronize on ONE single-pair 4K context, direction FORWARD and BACKWARD in turn (each direction has
    its own captured graph), taking turns to go first; with the speculative search on (the default of a single pair) and off.
    Controls: each direction repeated on its own (no alternation), and a context of its own fed the exchanged pair, which runs
    the backward problem in direction FORWARD."""
    w, h, search, block, levels = SHAPES["4k_4x2"][:5]
    f = bbme.synth_video(w, h, 2, 4242, max_motion=8)
    ss, bs = [search] * levels, [block] * levels

    def timed(mf, back=None):
        if back is not None:
            mf.set_direction(back)
        t0 = time.perf_counter()
        mf.estimate_async()
        mf.synchronize()
        return time.perf_counter() - t0

    for spec in (True, False):
        mf = bbme.MF(f[0], f[1], ss, bs, levels, device=device)
        ex = bbme.MF(f[1], f[0], ss, bs, levels, device=device)
        for m in (mf, ex):
            m.set_speculation(spec)
        for _ in range(3):
            timed(ex)
            for back in ((True, False) if backward_first else (False, True)):
                timed(mf, back)
        what = "direction, 4K single pair (search %d, block %d, %d levels), speculation %s" % (search, block, levels, "on" if spec else "off")
        if backward_first:
            what += ", BACKWARD captured first"
        for run in range(2):
            t = {False: [], True: [], "ex": []}
            for k in range(reps):
                for back in ((False, True) if k % 2 == 0 else (True, False)):
                    t[back].append(timed(mf, back))
                t["ex"].append(timed(ex))
            (mf_, minf), (mb_, minb), (me_, mine) = median_min(t[False]), median_min(t[True]), median_min(t["ex"])
            print("%s, run %d, %d alternating estimates: FORWARD %.4f ms median (min %.4f)   BACKWARD %.4f ms median (min %.4f)   "
                  "backward/forward %.4f   exchanged pair on its own context, FORWARD %.4f ms median (min %.4f)" %
                  (what, run + 1, reps, mf_, minf, mb_, minb, mb_ / mf_, me_, mine))
        for back in (False, True):
            t = [timed(mf, back) for _ in range(reps)]
            print("%s, %s repeated %d times: %.4f ms median (min %.4f)" % (what, "BACKWARD" if back else "FORWARD", reps, *median_min(t)))
        mf.close()
        ex.close()


def run_kernel(device, reps):
    import torch
    w, h, search, block, levels = SHAPES["4k_4x6"][:5]
    pairs = 6
    f = bbme.synth_video(w, h, pairs + 1, 4242, max_motion=8)
    chain = bbme.MFChain(f, [search] * levels, [block] * levels, levels, device=device)
    chain.set_speculation(False)
    chain.estimate_bidirectional_async()
    chain.synchronize()
    CH, CW = chain.cells_shape
    lib = _capi.lib()
    pa, pb = C.c_void_p(), C.c_void_p(chain.backward_cells_device_ptr(0))
    _capi.check(lib.bbme_cells_device_pair(chain._ctx, 0, C.byref(pa)))
    mask = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    pm, ps = C.c_void_p(mask.data_ptr()), C.c_void_p(st.data_ptr())
    torch.cuda.synchronize()
    for m, s in ((pm, None), (None, ps), (pm, ps)):
        for _ in range(reps):
            _capi.check(lib.bbme_cells_consistency_device(chain._ctx, pa, pb, 1, None, m, CW, s, None))
        chain.synchronize()
    for _ in range(reps):
        all_stats = chain.consistency_stats_all("forward", 1, "all")
    plane = torch.zeros((chain.padded_height, chain.padded_width), dtype=torch.uint8, device="cuda")
    for _ in range(reps):
        chain.motion_compensated_device(plane, 0, 2, 0)
    chain.synchronize()
    one = tuple(int(v) for v in st.cpu().numpy())
    assert one == tuple(all_stats[0][k] for k in ("consistent", "inconsistent", "outside", "discrepancy"))
    assert np.array_equal(mask.cpu().numpy(), chain.consistency("forward", 1))
    print("kernel run: %dx%d padded, %d x %d cells, %d launches per variant; pair 0 at tolerance 1: %s" %
          (chain.padded_width, chain.padded_height, CW, CH, reps, all_stats[0]))
    print("  per pair: reads 2 x 4 x %d = %d B, writes %d B" % (CH * CW, 8 * CH * CW, CH * CW))
    chain.close()


def report(trace_dir, reps):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def times(sub):
        return [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if sub in r["Kernel_Name"]]
    fb = times("k_fb_consistency")
    # the estimate launches none; the run's own checks add one mask launch at the end
    for i, name in enumerate(KERNEL_VARIANTS):
        t = sorted(fb[i * reps:(i + 1) * reps])
        if t:
            print("k_fb_consistency, %-26s %d launches: median %.2f us, min %.2f us" % (name + ":", len(t), t[len(t) // 2] / 1e3, t[0] / 1e3))
    mc = sorted(times("k_motion_compensate")[-reps:])
    if mc:
        print("k_motion_compensate, frame only, 1 pair: %d launches: median %.2f us, min %.2f us" % (len(mc), mc[len(mc) // 2] / 1e3, mc[0] / 1e3))
    red = sorted(times("k_mc_reduce"))
    if red:
        print("k_mc_reduce: %d launches: median %.2f us, min %.2f us" % (len(red), red[len(red) // 2] / 1e3, red[0] / 1e3))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--direction", action="store_true")
    ap.add_argument("--backward-first", action="store_true", help="--direction: capture the BACKWARD graph before the FORWARD one")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--report", metavar="DIR")
    a = ap.parse_args()
    if a.report:
        return report(a.report, a.reps)
    if a.kernel:
        return run_kernel(a.device, a.reps)
    if a.direction:
        return run_direction(a.device, a.reps, a.backward_first)
    print("both fields of a video's pairs, two-pass vs one-pass; every figure from %d timed rounds after 3 warm-up rounds, "
          "(a) and (b) alternating" % a.rounds)
    for name in [s for s in a.shapes.split(",") if s]:
        run_shape(name, SHAPES[name], a.rounds, a.device)


if __name__ == "__main__":
    main()
