"""The consecutive pairs of a video two ways, on the same seeded video and the same shape of contexts:

  (a) pairs   batched contexts (MFBatch) fed pair by pair: both frames of every pair are uploaded, padded and run through the
              pyrDown cascade -- every inner frame of the video twice -- with num_levels preparation launches PER PAIR
  (b) chain   chain contexts (MFChain): a round rolls the context's last frame to slot 0 on the GPU and sets the P new frames
              as ONE run -- every frame once, num_levels preparation launches (+ the roll) PER ROUND

Every context walks its own contiguous segment of the video (sequence.plan_frame_segments' dealing), `contexts` x `pairs`
pairs per round; a round = set the frames of every context and enqueue its estimate, then download every pair's cells.  Wall
milliseconds per pair on the host clock around that synchronised work, (a) and (b) alternating round by round in one process
after warm-up, for pinned and for pageable host frames, each measurement made twice to show the spread; the bytes each form
moves up (from the shapes); an assertion that every field of (a) equals (b)'s.  Then the estimate alone (frames resident,
estimate_async + synchronize) on a chain context against a batched context of the same P, alternating (and taking turns to
go first), in five blocks with fresh contexts each: the two run the same kernels with the same address arithmetic and must
agree within the spread the batched contexts show among themselves.

  python scripts/video_pipeline.py [--rounds 20] [--device 0] [--shapes 4k_4x2,4k_4x6,1080p_4x8] [--estimate-only]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/video_pipeline.py --trace     # launch counts, kernel times

--trace: no timing; per shape exactly `--trace-rounds` rounds of each form after the contexts' first frames, and the number
of launches of every preparation kernel that this must show in the trace's statistics.
"""
import argparse
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blockbasedmotionestimation_amd as bbme  # noqa: E402
from blockbasedmotionestimation_amd import _capi  # noqa: E402

SHAPES = {
    # name: width, height, search, block, levels, contexts, pairs per context
    "4k_4x2": (3840, 2160, 80, 16, 4, 4, 2),          # cfg3's parameters
    "4k_4x6": (3840, 2160, 80, 16, 4, 4, 6),
    "1080p_4x8": (1920, 1080, 48, 16, 3, 4, 8),       # cfg2's
}
POOL = 13            # distinct frames; the video walks them back and forth, so consecutive frames always differ by real motion


def median_min(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3


def pinned_like(frames):
    import torch
    keep = [torch.empty(f.shape, dtype=torch.uint8).pin_memory() for f in frames]
    views = []
    for t, f in zip(keep, frames):
        v = t.numpy()
        v[...] = f
        views.append(v)
    return views, keep


class Video:
    """Frame k of an endless video over a pool of frames: 0, 1, ..., n-1, n-2, ..., 1, 0, 1, ..."""

    def __init__(self, pool):
        self.pool = pool

    def __getitem__(self, k):
        n = len(self.pool)
        k %= 2 * n - 2
        return self.pool[k if k < n else 2 * n - 2 - k]


class Forms:
    """The two forms over `contexts` contexts of `pairs` pairs; context c starts at frame c * stride of the video."""

    def __init__(self, shape, video, device, stride):
        w, h, search, block, levels, self.contexts, self.pairs = shape
        self.w, self.h, self.video, self.stride = w, h, video, stride
        ss, bs = [search] * levels, [block] * levels
        first = [[video[c * stride + i] for i in range(self.pairs + 1)] for c in range(self.contexts)]
        self.batched = [bbme.MFBatch(list(zip(f, f[1:])), ss, bs, levels, device=device) for f in first]
        self.chains = [bbme.MFChain(f, ss, bs, levels, device=device) for f in first]
        for mf in self.batched + self.chains:
            mf.set_speculation(False)                  # several pairs in flight fill the chip already
        shape_c = (self.batched[0].padded_height // 2, self.batched[0].padded_width // 2, 2)
        import torch
        self._keep = [torch.empty((self.contexts, self.pairs) + shape_c, dtype=torch.int16).pin_memory() for _ in range(2)]
        self.cells = [t.numpy() for t in self._keep]   # [form][context, pair]
        self.levels = levels

    def close(self):
        for mf in self.batched + self.chains:
            mf.close()

    def frames_of_round(self, c, r):
        k = c * self.stride + r * self.pairs
        return [self.video[k + i] for i in range(self.pairs + 1)]

    def round_pairs(self, r):
        lib = _capi.lib()
        for c, mf in enumerate(self.batched):
            f = self.frames_of_round(c, r)
            for p in range(self.pairs):
                _capi.check(lib.bbme_set_frames_host_async(mf._ctx, p, f[p].ctypes.data, f[p + 1].ctypes.data, self.w))
            mf.estimate_async()
        for c, mf in enumerate(self.batched):
            for p in range(self.pairs):
                mf.get_pair_cells(p, out=self.cells[0][c, p])

    def round_chain(self, r):
        for c, mf in enumerate(self.chains):
            mf.advance(self.frames_of_round(c, r)[1:], wait=False)
            mf.estimate_async()
        for c, mf in enumerate(self.chains):
            for p in range(self.pairs):
                mf.get_pair_cells(p, out=self.cells[1][c, p])

    def check_round(self, r, what):
        if not np.array_equal(self.cells[0], self.cells[1]):
            bad = [(c, p) for c in range(self.contexts) for p in range(self.pairs)
                   if not np.array_equal(self.cells[0][c, p], self.cells[1][c, p])]
            raise AssertionError("%s, round %d: the fields of (a) and (b) differ for (context, pair) %s" % (what, r, bad))
        return zlib.crc32(self.cells[0].tobytes())


def timed_rounds(forms, first_round, rounds, what):
    ta, tb, crc = [], [], 0
    for r in range(first_round, first_round + rounds):
        t0 = time.perf_counter()
        forms.round_pairs(r)
        t1 = time.perf_counter()
        forms.round_chain(r)
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
        crc ^= forms.check_round(r, what)              # outside both timers
    n = forms.contexts * forms.pairs
    return [x / n for x in ta], [x / n for x in tb], crc


def estimate_alone(shape, video, device, reps, blocks=5):
    """Medians (and minima) of ms per pair of `blocks` blocks of `reps` alternating estimates.  Every block has a batched and a
    chain context of its own, created while the earlier blocks' contexts still hold their memory: where hipMalloc puts the
    planes moves either kind of context by about a percent (a batched context measured 1.095 - 1.109 ms per pair over six
    processes at 4K, 2 pairs, while three blocks on ONE context stay within 0.002 ms), so the spread that says whether two
    layouts differ is the one over fresh contexts, not over repeats on the same one."""
    w, h, search, block, levels, _, pairs = shape
    ss, bs = [search] * levels, [block] * levels
    f = [video[i] for i in range(pairs + 1)]
    out, alive = [], []
    for _ in range(blocks):
        batched = bbme.MFBatch(list(zip(f, f[1:])), ss, bs, levels, device=device)
        chain = bbme.MFChain(f, ss, bs, levels, device=device)
        alive += [batched, chain]
        for mf in (batched, chain):
            mf.set_speculation(False)
        for _ in range(3):
            for mf in (batched, chain):
                mf.estimate_async()
                mf.synchronize()
        for p in range(pairs):
            assert np.array_equal(batched.get_pair_cells(p), chain.get_pair_cells(p))
        t = {0: [], 1: []}
        for k in range(reps):
            # batched, chain / chain, batched in turn: whatever the second of two back-to-back estimates gains or loses
            # (caches, clocks) falls on both alike
            for i, mf in ((0, batched), (1, chain))[::1 if k % 2 == 0 else -1]:
                t0 = time.perf_counter()
                mf.estimate_async()
                mf.synchronize()
                t[i].append((time.perf_counter() - t0) / pairs)
        out.append((median_min(t[0]), median_min(t[1])))
    for mf in alive:
        mf.close()
    return out


def run_shape(name, shape, rounds, device, estimate_only=False):
    w, h, search, block, levels, contexts, pairs = shape
    pool = bbme.synth_video(w, h, POOL, 4242, max_motion=8)
    stride = 2 * pairs + 1
    lines = []
    per_round = contexts * pairs
    up_a = 2 * w * h
    up_b_first = (pairs + 1) * w * h / pairs
    lines.append("%s: %dx%d, search %d, block %d, %d levels; %d contexts x %d pairs = %d pairs per round; %d timed rounds per figure" %
                 (name, w, h, search, block, levels, contexts, pairs, per_round, rounds))
    lines.append("  upload per pair (from the shapes): (a) %d B = 2 W H;  (b) %d B = W H after a context's first round "
                 "(%d B per pair in that round)" % (up_a, w * h, up_b_first))
    lines.append("  preparation launches per context and round (from the call sequence): (a) %d = num_levels x P;  (b) %d = num_levels, + 1 roll" %
                 (levels * pairs, levels))
    pinned, keep = pinned_like(pool) if not estimate_only else (None, None)
    for kind, frames in (("pinned", pinned), ("pageable", pool)) if not estimate_only else ():
        forms = Forms(shape, Video(frames), device, stride)
        nxt = 1
        for r in range(nxt, nxt + 3):                  # warm-up: graphs captured, buffers allocated
            forms.round_pairs(r)
            forms.round_chain(r)
            forms.check_round(r, name)
        nxt += 3
        for rep in range(2):
            ta, tb, crc = timed_rounds(forms, nxt, rounds, "%s, %s frames" % (name, kind))
            nxt += rounds
            (ma, mina), (mb, minb) = median_min(ta), median_min(tb)
            lines.append("  %-8s frames, run %d: (a) pairs %7.3f ms/pair median (min %.3f)   (b) chain %7.3f ms/pair median (min %.3f)   "
                         "(a)/(b) %.2f   fields equal: yes (crc %08x)" % (kind, rep + 1, ma, mina, mb, minb, ma / mb, crc))
        forms.close()
    del keep
    blocks = estimate_alone(shape, Video(pool), device, rounds)
    bat = [b[0][0] for b in blocks]
    cha = [b[1][0] for b in blocks]
    spread = max(bat) - min(bat)
    gap = abs(sorted(cha)[len(cha) // 2] - sorted(bat)[len(bat) // 2])
    lines.append("  estimate alone, ms/pair, medians of %d blocks of %d alternating estimates, fresh contexts per block:" % (len(blocks), rounds))
    lines.append("    batched %s   (minima %s)" % (" ".join("%.4f" % v for v in bat), " ".join("%.4f" % b[0][1] for b in blocks)))
    lines.append("    chain   %s   (minima %s)" % (" ".join("%.4f" % v for v in cha), " ".join("%.4f" % b[1][1] for b in blocks)))
    lines.append("    batched contexts' spread over blocks %.4f ms; |median chain - median batched| %.4f ms: %s" %
                 (spread, gap, "within the spread" if gap <= spread else "OUTSIDE the spread"))
    return lines


def run_trace(name, shape, rounds, device):
    w, h, search, block, levels, contexts, pairs = shape
    pool = bbme.synth_video(w, h, POOL, 4242, max_motion=8)
    forms = Forms(shape, Video(pool), device, 2 * pairs + 1)
    for r in range(1, 1 + rounds):
        forms.round_pairs(r)
        forms.round_chain(r)
        forms.check_round(r, name)
    forms.close()
    # creation: MFBatch sets P pairs, MFChain one run; then `rounds` rounds of each
    # (one launch per setter and level: P pair setters of the batched form, one run setter of the chain)
    n = {"k_pad_zero_run": contexts * (pairs + 1) * (1 + rounds), "k_pyr_down4_run": contexts * (pairs + 1) * (1 + rounds) * (levels - 1),
         "k_chain_roll": contexts * rounds}
    print("%s: %d contexts x %d pairs, %d levels, %d rounds of each form after the contexts' first frames" %
          (name, contexts, pairs, levels, rounds))
    print("  expected launches: " + ", ".join("%s %d" % kv for kv in n.items()))
    print("  per context and round: (a) %d preparation launches, (b) %d + 1 roll" % (levels * pairs, levels))
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--estimate-only", action="store_true", help="only the estimate-alone comparison")
    ap.add_argument("--trace-rounds", type=int, default=4)
    a = ap.parse_args()
    names = [s for s in a.shapes.split(",") if s]
    if a.trace:
        total = {}
        for name in names:
            for k, v in run_trace(name, SHAPES[name], a.trace_rounds, a.device).items():
                total[k] = total.get(k, 0) + v
        print("expected launches in all: " + ", ".join("%s %d" % kv for kv in total.items()))
        return
    print("video pipeline, pairs vs chain; every figure from %d timed rounds after 3 warm-up rounds, (a) and (b) alternating" % a.rounds)
    for name in names:
        for line in run_shape(name, SHAPES[name], a.rounds, a.device, a.estimate_only):
            print(line)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
