"""CPU side of the global-motion scale tests (tests/test_gpu_scale.py): what SCALE_G1, GM_WIDE and GM_TALL make K16
k_vector_histogram, K17 k_global_moments with k_reduce_words<16>, K18 k_global_compensate and K18b k_global_compensate_bgr do --
recomputed here from the kernels' own constants, so that a change to one of them or to a shape fails without a GPU -- and the
generated content, put through the numpy rules alone, is not trivial: every class of the moments in bulk, sums of products beyond
2^40 and 2^31, one histogram bin beyond 2^17, compensation that skips and sums beyond 2^32.  The host mirrors equal numpy at the
two new shapes, so that a GPU mismatch there points at the kernel and not at the rule."""
import os
import re

import numpy as np
import pytest

import helpers as H
from test_global_compensation_bgr_cpu import np_global_compensate_bgr
from test_global_motion_cpu import (COMP_MODELS, MODELS, STAT_KEYS, np_global_compensate, np_histogram, np_moments)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blockbasedmotionestimation_amd", "csrc")
NAMES = ("G1", "WIDE", "TALL")


def constants():
    """kVhMaxGroups, the three runs-per-lane constants and the slices of the k_reduce_words<16> that K17's launch names"""
    kernels = open(os.path.join(CSRC, "bbme_kernels.hpp")).read()
    device = open(os.path.join(CSRC, "bbme_device.hip")).read()
    found = dict(re.findall(r"constexpr int k(VhMaxGroups|GmRunsPerLane|GcRunsPerLane|GcBgrRunsPerLane) = (\d+);", kernels))
    assert sorted(found) == ["GcBgrRunsPerLane", "GcRunsPerLane", "GmRunsPerLane", "VhMaxGroups"], found
    assert "constexpr int kSlices = 256 / WORDS;" in kernels and "for (int g = slice; g < groups; g += kSlices)" in kernels
    words = set(re.findall(r"k_reduce_words<(\d+)>", device))
    assert words == {"16"}, words
    out = {k: int(v) for k, v in found.items()}
    out["Slices"] = 256 // 16
    return out


def padded(bbme, name):
    g = H.GM_SHAPES[name]
    return bbme.plan_padding(g["w"], g["h"], g["search"], g["block"])


def test_the_kernels_constants_are_the_ones_the_shapes_were_derived_from():
    assert constants() == {"VhMaxGroups": 256, "GmRunsPerLane": 4, "GcRunsPerLane": 4, "GcBgrRunsPerLane": 4, "Slices": 16}


def test_shapes_reach_the_strided_loop_the_second_reduction_trip_and_257_partials(bbme):
    k = constants()
    for name in NAMES:
        assert tuple(padded(bbme, name)) == H.GM_PADDED[name] + (1, 1), name
    # K16: (runs, workgroups, trips, runs of the last trip)
    vh = {name: H.gm_trips(*H.GM_PADDED[name], k["VhMaxGroups"]) for name in NAMES}
    assert vh == {"G1": (134160, 256, 3, 3088), "WIDE": (67584, 256, 2, 2048), "TALL": (69598, 256, 2, 4062)}
    assert all(trips > 1 for _, _, trips, _ in vh.values())                     # the loop `base += gridDim.x * 256` goes round
    assert any(trips >= 3 for _, _, trips, _ in vh.values())
    assert any(last % 256 for _, _, _, last in vh.values())                     # a last trip that ends inside a workgroup:
    assert vh["TALL"][3] == 15 * 256 + 222 and vh["G1"][3] == 12 * 256 + 16     # lanes past `runs` next to live ones, whole waves
    assert vh["WIDE"][3] % 256 == 0                                             # of them at G1, a part of a wave at GM_TALL
    # K17: (runs, workgroups, runs in the last workgroup), and the trips of k_reduce_words<16>
    gm = {name: H.scale_groups(*H.GM_PADDED[name], k["GmRunsPerLane"]) for name in NAMES}
    assert {n: v[1] for n, v in gm.items()} == {"G1": 132, "WIDE": 66, "TALL": 68}
    for name, (_, groups, _) in gm.items():
        assert groups > k["Slices"] and groups % k["Slices"], name              # a second trip, and an uneven last one
    assert -(-gm["G1"][1] // k["Slices"]) == 9
    # K18 and K18b: at least 257 partials, so that a lane of k_mc_reduce takes a second trip
    gc = {name: H.scale_groups(*H.GM_PADDED[name], k["GcRunsPerLane"], cells=False) for name in NAMES}
    assert {n: v[1] for n, v in gc.items()} == {"G1": 524, "WIDE": 264, "TALL": 264}
    gcb = {name: H.scale_groups(H.GM_SHAPES[name]["w"], H.GM_SHAPES[name]["h"], k["GcBgrRunsPerLane"], cells=False) for name in ("G1", "WIDE")}
    assert {n: v[1] for n, v in gcb.items()} == {"G1": 523, "WIDE": 260}
    assert all(v[1] >= 257 for v in list(gc.values()) + list(gcb.values()))
    for last, rpl in ((gc["G1"][2], k["GcRunsPerLane"]), (gcb["G1"][2], k["GcBgrRunsPerLane"])):
        assert 0 < last < 256 * rpl                                             # a part-filled last workgroup at SCALE_G1
    # the rule's limit, and rows that end in a run of 2 cells
    assert H.GM_PADDED["WIDE"][0] == 8188 and H.GM_PADDED["TALL"][1] == 8188
    assert (H.GM_PADDED["WIDE"][0] // 2) % 4 == 2 and (H.GM_PADDED["TALL"][0] // 2) % 4 == 2


@pytest.mark.parametrize("name", NAMES)
def test_moments_content_fills_every_class_and_passes_32_bits(bbme, name):
    w0, h0 = H.GM_PADDED[name]
    ch, cw = h0 // 2, w0 // 2
    g, model, mask = H.gm_scale_grid(ch, cw)
    window = H.gm_cell_window(cw, ch)
    cls, words = np_moments(g, model, H.GM_TOL, mask, window)
    cells = window[2] * window[3]
    bits = [int(abs(int(v))).bit_length() for v in words]
    print("%s: classes %s of %d cells, bits per word %s" % (name, words[:3].tolist(), cells, bits))
    assert words[:3].sum() == cells and all(n >= cells // 4 for n in words[:3]), words[:3]
    if name == "G1":                                               # |X| <= 2059 there: beyond 32 bits, which is what a narrow sum loses
        assert max(abs(int(v)) for v in words[6:9]) >= 2 ** 32
    else:
        assert max(abs(int(v)) for v in words[6:9]) >= 2 ** 40
        assert max(abs(int(v)) for v in words[11:15]) >= 2 ** 31
    # the int32-extreme models leave inliers too, under the widest tolerance
    for m in MODELS[3:5]:
        _, w = np_moments(g, m, 2 ** 40, mask, window)
        assert w[0] > 0 and w[1] > w[0] and int(w[3]).bit_length() > 40, (m, w)
    if name != "G1":
        got_map, got = bbme.global_moments_cells(g, model, H.GM_TOL, mask, window)
        assert np.array_equal(got_map, cls) and np.array_equal(got, words)
        for m in MODELS[3:5]:
            got_map, got = bbme.global_moments_cells(g, m, 2 ** 40)
            exp_map, exp = np_moments(g, m, 2 ** 40)
            assert np.array_equal(got_map, exp_map) and np.array_equal(got, exp), m


@pytest.mark.parametrize("name", NAMES)
def test_histogram_content_puts_every_cell_into_one_bin(bbme, name):
    w0, h0 = H.GM_PADDED[name]
    ch, cw = h0 // 2, w0 // 2
    grids, mask = H.gm_histogram_grids(ch, cw)
    window = H.gm_cell_window(cw, ch)
    for gname, g in grids:
        hist = np_histogram(g)
        if gname == "uniform":
            assert hist.max(axis=1).tolist() == [ch * cw] * 2 and ch * cw > 2 ** 17
        else:
            assert (hist > 0).sum() >= 2 * 7
        if name != "G1":
            assert np.array_equal(bbme.vector_histogram_cells(g), hist), gname
            assert np.array_equal(bbme.vector_histogram_cells(g, mask, window), np_histogram(g, mask, window)), gname


@pytest.mark.parametrize("name", NAMES)
def test_compensation_content_skips_and_sums_beyond_32_bits(bbme, name):
    w0, h0 = H.GM_PADDED[name]
    I1, I2 = H.gm_scale_planes(h0, w0)
    both = beyond = 0
    for k, (model, unit) in enumerate(COMP_MODELS[:4]):
        out, st = np_global_compensate(I1, I2, model, unit, 7)
        share = st[2] / float(w0 * h0)
        print("%s: model %d compensates %.1f %%, sse %d" % (name, k, 100 * share, st[0]))
        both += 0.25 <= share <= 0.75
        beyond += st[0] > 2 ** 32
        if name != "G1":
            got, gst = bbme.global_compensate(I1, I2, model, unit, 7)
            assert np.array_equal(got, out) and tuple(gst[s] for s in STAT_KEYS) == st, k
    assert both >= 1 and beyond >= 1
    if name != "G1":
        win = H.gm_plane_window(w0, h0)
        model, unit = COMP_MODELS[1]
        got, gst = bbme.global_compensate(I1, I2, model, unit, 9, win)
        exp, st = np_global_compensate(I1, I2, model, unit, 9, win)
        assert np.array_equal(got, exp) and tuple(gst[s] for s in STAT_KEYS) == st


@pytest.mark.parametrize("name", ("G1", "WIDE"))
def test_colour_compensation_content_and_its_host_rule(bbme, name):
    """The GPU test holds K18b against the host rule: here the host rule against numpy on the same frames, models and window"""
    g = H.GM_SHAPES[name]
    c1, c2, models, unit, window = H.gm_scale_bgr_case(g["h"], g["w"])
    stats = []
    for k in range(3):
        out, st = bbme.global_compensate_bgr(c1[k], c2[k], models[k], unit, 3, 1, 1, window)
        exp, exp_st = np_global_compensate_bgr(c1[k], c2[k], models[k], unit, 3, 1, 1, window)
        assert np.array_equal(out, exp) and tuple(st[s] for s in STAT_KEYS) == exp_st, k
        stats.append(exp_st)
    assert H.stats_differ_pairwise(stats, words=(0, 1)), stats
    assert all(s[0] > 2 ** 32 for s in stats) and any(s[3] > 0 for s in stats)
