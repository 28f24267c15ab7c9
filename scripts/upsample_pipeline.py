"""The reference's x4 pipeline (main_class.cpp:32-33, 45-70) two ways, per frame pair:

  (a) host  bbme_resize_x4_host x2 -> bbme_set_frames_host -> estimate -> bbme_get_flow_host (dense padded field)
            -> bbme_subsample_div4
  (b) x4    bbme_set_frames_host_x4 (original frames) -> estimate -> bbme_get_subsampled_flow_host

Wall milliseconds per pair on the host clock around synchronised work (every call in both pipelines returns only when its
result is on the host), after warm-up, from pageable numpy buffers; the bytes each pipeline moves across PCIe; and a check
that both give the same field.  Usage: python scripts/upsample_pipeline.py [--reps N] [--device D]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import blockbasedmotionestimation_amd as bbme  # noqa: E402

CASES = [
    # name, source width, height, search, block, levels
    ("ref", 584, 388, 64, 32, 4, "reference literals (main_class.cpp:19-21), 584x388 -> 2336x1552"),
    ("cfg3_src", 960, 540, 80, 16, 4, "cfg3 parameters, 960x540 -> 3840x2160"),
]


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return stats(out)


def run_case(name, w, h, search, block, levels, desc, reps, device):
    f1, f2, _ = bbme.synth_pair(w, h, 4242, max_motion=12)
    ss, bs = [search] * levels, [block] * levels
    u1, u2 = bbme.resize_x4(f1), bbme.resize_x4(f2)
    host = bbme.MF(u1, u2, ss, bs, levels, device=device)
    x4 = bbme.MF(f1, f2, ss, bs, levels, device=device, upsample=4)
    px, py = host.padding_x, host.padding_y
    res = {}

    def pipeline_a():
        a1, a2 = bbme.resize_x4(f1), bbme.resize_x4(f2)
        host.set_frames(a1, a2)
        host.estimate_async()
        res["a"] = bbme.subsample_div4(host.get_flow(), px, py, w, h)

    def pipeline_b():
        x4.set_frames(f1, f2)
        x4.estimate_async()
        res["b"] = x4.get_subsampled_flow()

    def estimate_only():
        x4.estimate_async()
        x4.synchronize()

    for _ in range(3):
        pipeline_a()
        pipeline_b()
    assert np.array_equal(res["a"], res["b"]), "%s: the two pipelines disagree" % name
    ta = timed(pipeline_a, reps)
    tb = timed(pipeline_b, reps)
    tr = timed(lambda: (bbme.resize_x4(f1), bbme.resize_x4(f2)), reps)
    flow = host.get_flow()
    ts = timed(lambda: bbme.subsample_div4(flow, px, py, w, h), reps)
    te = timed(estimate_only, reps)
    assert np.array_equal(res["a"], res["b"]), "%s: the two pipelines disagree" % name
    up_a, up_b = 2 * (4 * w) * (4 * h), 2 * w * h
    down_a, down_b = host.padded_width * host.padded_height * 8, w * h * 8
    host.close()
    x4.close()
    lines = ["%s: %s, search %d, block %d, %d levels; padded %dx%d" % (name, desc, search, block, levels,
                                                                      host.padded_width, host.padded_height),
             "  (a) host resize + dense download : %8.3f ms/pair median (min %.3f)   PCIe up %9d B, down %9d B" %
             (ta[0], ta[1], up_a, down_a),
             "  (b) x4 on the GPU, subsampled    : %8.3f ms/pair median (min %.3f)   PCIe up %9d B, down %9d B" %
             (tb[0], tb[1], up_b, down_b),
             "      speed-up (a)/(b), medians    : %8.2f x" % (ta[0] / tb[0]),
             "  parts of (a): host resize_x4 of both frames %.3f ms, host subsample_div4 %.3f ms" % (tr[0], ts[0]),
             "  estimate alone (enqueue + synchronise, x4 context): %.3f ms" % te[0],
             "  outputs identical: yes (%d x %d x 2 float32)" % (h, w)]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    print("x4 pipeline, host vs GPU; %d timed pairs per figure after 3 warm-up pairs; pageable host buffers" % a.reps)
    for c in CASES:
        for line in run_case(*c, reps=a.reps, device=a.device):
            print(line)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
