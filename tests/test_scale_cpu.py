"""CPU side of the scale tests (tests/test_gpu_scale.py): the two shapes are the smallest at which every gather kernel leaves more
than 256 partials per pair with a last workgroup that is only partly filled -- recomputed here from the kernels' own constants, so
that a change to either fails without a GPU -- and the generated content, put through the numpy rules alone, is not trivial: every
temporal weight, every interpolation hypothesis and every consistency class occurs in bulk, compensation skips and sums beyond
2^32, and results that share a launch differ in every word."""
import os
import re

import numpy as np
import pytest

import helpers as H
from test_consistency_cpu import np_cells_consistency
from test_interpolation_cpu import np_interpolate
from test_motion_compensation_cpu import block_mvs_from_grid, np_draw_mvimage, np_stats
from test_temporal_filter_cpu import np_temporal_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc", "bbme_kernels.hpp")


def runs_per_lane():
    text = open(KERNELS).read()
    found = dict(re.findall(r"constexpr int k(Mc|Fb|Ip|Tf)RunsPerLane = (\d+);", text))
    assert sorted(found) == ["Fb", "Ip", "Mc", "Tf"], found
    return {k: int(v) for k, v in found.items()}


def padded(bbme, g):
    return bbme.plan_padding(g["w"], g["h"], g["search"], g["block"])


def test_the_kernels_constants_are_the_ones_the_shapes_were_derived_from():
    assert runs_per_lane() == {"Mc": 4, "Fb": 4, "Ip": 2, "Tf": 2}


def test_shapes_reach_the_second_trip_of_the_reduction(bbme):
    k = runs_per_lane()
    assert tuple(padded(bbme, H.SCALE_G1)) == (2060, 1040, 1, 1)
    assert tuple(padded(bbme, H.SCALE_G2)) == (2060, 2072, 1, 1)
    w1, h1 = padded(bbme, H.SCALE_G1)[:2]
    w2, h2 = padded(bbme, H.SCALE_G2)[:2]
    assert (w1 // 2, h1 // 2) == (1030, 520) and (w1 // 2 + 3) // 4 == 258
    # (kernel, shape it is tested at, runs per lane, cells or pixels): (runs, workgroups, runs in the last workgroup)
    expected = {
        ("k_interpolate", "G1"): (134160, 263, 16), ("k_temporal_filter", "G1"): (134160, 263, 16),
        ("k_motion_compensate", "G1"): (535600, 524, 48), ("k_fb_consistency", "G2"): (267288, 262, 24),
    }
    got = {
        ("k_interpolate", "G1"): H.scale_groups(w1, h1, k["Ip"]), ("k_temporal_filter", "G1"): H.scale_groups(w1, h1, k["Tf"]),
        ("k_motion_compensate", "G1"): H.scale_groups(w1, h1, k["Mc"], cells=False),
        ("k_fb_consistency", "G2"): H.scale_groups(w2, h2, k["Fb"]),
    }
    assert got == expected
    per_group = {"k_interpolate": 256 * k["Ip"], "k_temporal_filter": 256 * k["Tf"], "k_motion_compensate": 256 * k["Mc"],
                 "k_fb_consistency": 256 * k["Fb"]}
    for (kernel, shape), (runs, groups, last) in got.items():
        assert groups >= 257, (kernel, shape)                     # a lane of k_mc_reduce takes a second trip
        assert 0 < last < per_group[kernel], (kernel, shape)      # lanes of the last workgroup break out of the run loop
        assert last < 256, (kernel, shape)                        # ... whole waves of it among them
    for w0 in (w1, w2):
        assert (w0 // 2) % 4 == 2                                 # every cell row ends in a run of 2 cells
    assert H.scale_groups(w1, h1, k["Fb"])[1] == 132              # why consistency needs G2: one trip only at G1
    # odd paddings: the unpadded windows start at an odd pixel, and so do the cell windows
    default, odd = H.scale_cell_windows(1, 1, H.SCALE_G1["w"], H.SCALE_G1["h"])
    assert default == (1, 1, 1029, 519) and odd == (4, 2, 1021, 514)
    x0, y0, w, h = H.SCALE_MC_WINDOW
    assert x0 % 2 and y0 % 2 and (x0 + w) % 4 and (y0 + h) % 2 and x0 + w <= w1 and y0 + h <= h1


def test_temporal_filter_content_meets_every_weight(bbme):
    w0, h0 = padded(bbme, H.SCALE_G1)[:2]
    cur, prev, gp, nxt, gn = H.scale_filter_content(h0, w0)
    out, wmap, stats = np_temporal_filter(cur, prev, gp, nxt, gn, H.SCALE_STRENGTH)
    for name, weights in (("previous", wmap & 15), ("next", wmap >> 4)):
        counts = np.bincount(weights.reshape(-1), minlength=9)
        print("temporal filter, %s neighbour, cells per weight 0..8: %s" % (name, counts.tolist()))
        assert len(counts) == 9 and (counts >= 1000).all(), (name, counts)
    assert ((wmap[8:16] >> 4) == 0).all() and ((wmap[8:16] & 15) != 0).any()       # the one-sided rows
    assert (wmap[:8] == 0x88).all()
    assert stats[0] != stats[1] and (out != cur).mean() > 0.5


def test_interpolation_content_selects_every_hypothesis(bbme):
    w0, h0, px, py = padded(bbme, H.SCALE_G1)
    f1, f2 = H.scale_frames(H.SCALE_G1["h"], H.SCALE_G1["w"], 2)
    i1, i2 = bbme.pad_zero(f1, px, py), bbme.pad_zero(f2, px, py)
    fwd, bwd = H.scale_grids(h0 // 2, w0 // 2)
    _, odd = H.scale_cell_windows(px, py, H.SCALE_G1["w"], H.SCALE_G1["h"])
    cells = (h0 // 2) * (w0 // 2)
    stats = []
    for num in (1, 2, 3):                                         # the phases the GPU test takes from one launch
        _, sel, st = np_interpolate(i1, i2, fwd, bwd, num, 4, odd)
        counts = np.bincount(sel.reshape(-1), minlength=3)
        print("interpolation at %d / 4, cells per hypothesis: %s" % (num, counts.tolist()))
        assert (counts >= cells // 10).all(), (num, counts)
        stats.append(st)
    assert H.stats_differ_pairwise(stats), stats


def test_consistency_content_holds_every_class(bbme):
    w0, h0 = padded(bbme, H.SCALE_G2)[:2]
    a, b = H.scale_grids(h0 // 2, w0 // 2)
    cells = (h0 // 2) * (w0 // 2)
    stats = []
    for tol in (0, 1):
        _, st = np_cells_consistency(a, b, tol)
        print("consistency at tolerance %d: %s" % (tol, st))
        stats.append(st)
    assert all(n >= cells // 100 for n in stats[1][:3]), stats[1]
    assert stats[0][0] >= 1000 and stats[0][0] != stats[1][0]


def test_compensation_content_skips_and_sums_beyond_32_bits(bbme):
    g = H.SCALE_G1
    w0, h0, px, py = padded(bbme, g)
    f1, f2, grid = H.scale_mc_content(g["h"], g["w"], h0, w0, g["block"][0])
    i1, i2 = bbme.pad_zero(f1, px, py), bbme.pad_zero(f2, px, py)
    assert grid.shape == (h0 // 4, w0 // 4, 2)
    frame, ok = np_draw_mvimage(i2, block_mvs_from_grid(grid.astype(np.int32), 4, 4, h0, w0), 4, 0)
    sse, sad, pixels, skipped = np_stats(i1, frame, ok, H.SCALE_MC_WINDOW)
    print("compensation: sse %d sad %d pixels %d skipped %d" % (sse, sad, pixels, skipped))
    assert pixels > 0 and skipped > 0 and sse > 2 ** 32
    for rows, cols in ((slice(0, 16), slice(None)), (slice(h0 - 16, h0), slice(None)), (slice(None), slice(0, 16)),
                       (slice(None), slice(w0 - 16, w0))):
        assert not ok[rows, cols].all() and ok[rows, cols].any()  # blocks leave on all four sides


def test_video_content_moves_by_another_even_shift_per_frame_outside_a_rectangle():
    assert len(set(H.SCALE_SHIFTS)) == len(H.SCALE_SHIFTS)
    assert all(dy % 2 == 0 and dx % 2 == 0 and max(abs(dy), abs(dx)) <= 4 for dy, dx in H.SCALE_SHIFTS)   # within the search's +-4
    video = H.scale_video(64, 96, 4)
    for k in range(3):
        d = video[k + 1].astype(np.int64) - np.roll(video[k], H.SCALE_SHIFTS[k], axis=(0, 1))
        follows = (d >= 0) & (d <= 7)
        assert 0.5 < follows.mean() < 0.95, k                     # all but the frame's rectangle of unrelated noise


def test_pairs_of_the_video_share_no_statistic(bbme, oracle):
    """The batch and the chain of tests/test_gpu_scale.py on the oracle's fields (the kernels' own, bit for bit): whatever one
    launch computes for two pairs or two frames differs in every word, so a partial of the wrong pair cannot pass."""
    g = H.SCALE_G1
    video = H.scale_video(g["h"], g["w"], 4)
    assert all(np.array_equal(a, b) for a, b in zip(H.scale_video(g["h"], g["w"], 3), video))       # the chain's frames
    w0, h0, px, py = padded(bbme, g)
    default, _ = H.scale_cell_windows(px, py, g["w"], g["h"])
    planes = [bbme.pad_zero(f, px, py) for f in video]

    def cells(a, b):
        omf = oracle.OracleMF(video[a], video[b], g["search"], g["block"])
        H.oracle_schedule(omf, 1)
        out = omf.block_mvs(0, 2).astype(np.int16)
        omf.close()
        return out

    fwd = {p: cells(p, p + 1) for p in (0, 2)}
    bwd = {p: cells(p + 1, p) for p in (0, 2)}
    assert not np.array_equal(fwd[0], fwd[2]) and not np.array_equal(bwd[0], bwd[2])
    fb = [np_cells_consistency(fwd[p], bwd[p], 1, default)[1] for p in (0, 2)]
    assert H.stats_differ_pairwise(fb, absent_ok=True) and all(min(s[0], s[1], s[3]) > 0 for s in fb), fb
    mc = []
    for p in (0, 2):
        frame, ok = np_draw_mvimage(planes[p + 1], block_mvs_from_grid(fwd[p].astype(np.int32), 2, 4, h0, w0), 4, 0)
        mc.append(np_stats(planes[p], frame, ok, (px, py, g["w"], g["h"])))
    assert H.stats_differ_pairwise(mc, words=(0, 1)), mc
    ip = [np_interpolate(planes[p], planes[p + 1], fwd[p], bwd[p], 1, 2, default)[2] for p in (0, 2)]
    assert H.stats_differ_pairwise(ip), ip
    tf = []
    for p in (0, 2):
        tf.append(np_temporal_filter(planes[p], None, None, planes[p + 1], fwd[p], H.SCALE_STRENGTH, default)[2])
        tf.append(np_temporal_filter(planes[p + 1], planes[p], bwd[p], None, None, H.SCALE_STRENGTH, default)[2])
    assert H.stats_differ_pairwise(tf, absent_ok=True), tf
    print("consistency %s\ncompensation %s\ninterpolation %s\ntemporal filter %s" % (fb, mc, ip, tf))
