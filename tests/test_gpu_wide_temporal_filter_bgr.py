"""Temporal filtering of colour frames over two frames on each side on the GPU (include/bbme.h, "BGR WIDE TEMPORAL FILTER RULE"), all
bit-exact through the C-ABI: k_wide_temporal_filter_bgr gives the numpy restatement of tests/test_wide_temporal_filter_bgr_cpu.py
and the host rule on a caller's frames and grids -- every fraction, each of the 15 neighbour sets, geometries with odd paddings and
cut runs, colour and output pitches that reach the byte paths, map pitches that are no multiples of 4, strided grids, windows that
cut runs, a side stream, each output alone, every edge of the padded view and the int16 extremes under guard bands --; the division
by S is exact at every S in every channel; grey frames give k_wide_temporal_filter's bytes and two neighbours
k_subpel_temporal_filter_bgr's; colour chains of five and six frames filter every slot as the CPU route does on the oracle's luma
fields, chains of two and three slots degrade as the rule says; the calls need fields and stored colour, change no context state
and refuse bad arguments; sequence.denoise_frames_wide(bgr=True) filters every colour frame from every neighbour that exists."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _cuda, _odd_window, _status
from test_bgr_cpu import SHAPES, np_bgr_to_gray
from test_gpu_bgr import VIDEO, VIDEO_PARAMS, colour_video
from test_gpu_bidirectional import _oracle_fields
from test_gpu_temporal_filter_bgr import _colour7, _pitched_tensor
from test_interpolation_cpu import extreme_grids, odd_windows
from test_subpel_temporal_filter_bgr_cpu import edge_fraction_grid, grey3
from test_subpel_temporal_filter_cpu import edge_grid
from test_temporal_filter_cpu import STAT_KEYS
from test_wide_temporal_filter_bgr_cpu import (cpu_wide_bgr_route, flat_five, four_colour_frames, four_fraction_grids,
                                               np_wide_temporal_filter_bgr, weight_sums_in_channel)
from test_wide_temporal_filter_cpu import NEIGHBOUR_SETS, WIDE_KEYS, pick

pytestmark = pytest.mark.gpu

WHOLE_RUNS = (200, 136, (30, 30, 30), (16, 16, 16))        # pads to 256 x 192: whole runs, even paddings (28, 28)
GEOMETRIES = dict(SHAPES)
GEOMETRIES[WHOLE_RUNS] = (256, 192, 28, 28)


def _stats(d):
    return tuple(d[k] for k in WIDE_KEYS)


def _device_filter(mf, Cur, frames, grids, thr, window=None, colour_extra=0, out_extra=0, q_extra=0, map_extra=0, stream=None,
                   want=("out", "map", "stats")):
    """cells_temporal_filter_wide_bgr_device on host frames and grids -> (frame (H, W, 3), map (CH, CW) uint16, stats tuple), None
    where not asked for.  The colour frames' rows are colour_extra bytes, the output's rows out_extra bytes, the map's rows map_extra
    uint16 and every grid's rows q_extra cells further apart than packed; the bytes and cells in between and the 64 bytes behind the
    frame's last row stay untouched."""
    import torch
    CH, CW = mf.cells_shape
    h, w = mf.orig_height, mf.orig_width
    tc = _pitched_tensor(Cur, colour_extra)
    tf = [_pitched_tensor(f, colour_extra) for f in frames]
    tg = []
    for Q in grids:
        if Q is None:
            tg.append(None)
            continue
        t = torch.full((CH, CW + q_extra, 2), 0x7777, dtype=torch.int16, device="cuda")
        t[:, :CW] = _cuda(np.asarray(Q, np.int16))
        tg.append(t)
    pitch = 3 * w + out_extra
    raw = torch.full((h * pitch + 64,), 0xAA, dtype=torch.uint8, device="cuda") if "out" in want else None
    out = None if raw is None else raw.as_strided((h, w, 3), (pitch, 3, 1))
    wmap = torch.full((CH, CW + map_extra), 0x7AAA, dtype=torch.int16, device="cuda") if "map" in want else None
    st = torch.zeros(6, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    views = [None if t is None else (t[:, :CW] if q_extra else t[:, :CW].contiguous()) for t in tg]
    mf.cells_temporal_filter_wide_bgr_device(tc, tf, views, thr, out=out, weights=None if wmap is None else wmap[:, :CW], stats=st,
                                             window=window, stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    if raw is not None:
        rows = raw[:h * pitch].view(h, pitch)
        assert bool((rows[:, 3 * w:] == 0xAA).all()) and bool((raw[h * pitch - out_extra:] == 0xAA).all())
    assert wmap is None or not map_extra or bool((wmap[:, CW:] == 0x7AAA).all())
    for t in tg:
        assert t is None or bool((t[:, CW:] == 0x7777).all())
    return (None if out is None else out.cpu().numpy(), None if wmap is None else wmap[:, :CW].cpu().numpy().view(np.uint16),
            None if st is None else tuple(st.cpu().tolist()))


def _host(bbme, Cur, frames, grids, thr, px, py, window=None):
    out, wmap, st = bbme.temporal_filter_cells_wide_bgr(Cur, frames, grids, thr, px, py, window)
    return out, wmap, _stats(st)


def _assert_device_equals_numpy(mf, Cur, frames, grids, thr, window=None, what=None, host=None, **kw):
    """GPU = numpy (= the host rule where `host` is the package)"""
    out, wmap, st = _device_filter(mf, Cur, frames, grids, thr, window, **kw)
    px, py = mf.padding_x, mf.padding_y
    exp = np_wide_temporal_filter_bgr(Cur, frames, grids, thr, px, py, window)
    tag = (what, thr, [f is not None for f in frames], window)
    assert out is None or np.array_equal(out, exp[0]), tag
    assert wmap is None or np.array_equal(wmap, exp[1]), tag
    assert st is None or st == exp[2], tag
    if host is not None:
        h = _host(host, Cur, frames, grids, thr, px, py, window)
        assert np.array_equal(h[0], exp[0]) and np.array_equal(h[1], exp[1]) and h[2] == exp[2], tag
    return exp


def _check_edge_cells(exp, cells, Cur, px, py, chosen):
    """The valid cells took their neighbours; the others have weight 0 and keep C's pixels"""
    out, wmap = exp[:2]
    full, padC = (np.pad(f, ((py, py), (px, px), (0, 0))) for f in (out, Cur))
    for cx, cy, valid in cells:
        for k in range(4):
            assert (((wmap[cy, cx] >> (4 * k)) & 15) > 0) == (valid and k in chosen), (cx, cy, k, valid)
        if not valid:
            assert np.array_equal(full[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2], padC[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2])


@pytest.mark.parametrize("shape", list(GEOMETRIES))
def test_equals_numpy_and_the_host_rule(bbme, shape):
    import torch
    w, h, search, block = shape
    W0, H0, px, py = GEOMETRIES[shape]
    z = np.zeros((h, w, 3), np.uint8)
    mf = bbme.MF(z, z, list(search), list(block))
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == (W0, H0, px, py)
    CH, CW = mf.cells_shape
    assert CW % 4 == (0 if shape == WHOLE_RUNS or W0 == 128 else 2)
    cut = (CW - 7, 2, 7, CH - 5)                           # reaches the last run of the rows
    inner = (3, 1, 5, 3)                                   # starts and ends inside runs
    Cur, frames = four_colour_frames(w, h, 10 * h + w)
    grids = four_fraction_grids(H0, W0, 100 * W0 + H0)
    exp = _assert_device_equals_numpy(mf, Cur, frames, grids, 255, None, "fractions", host=bbme)
    every = {(a, b) for a in range(4) for b in range(4)}
    for k in range(4):                                     # every fraction class was taken, by every neighbour
        assert {(int(a) & 3, int(b) & 3) for a, b in grids[k][((exp[1] >> (4 * k)) & 15) > 0]} == every
    assert len({int(s) for s in 8 + sum((exp[1] >> (4 * k)) & 15 for k in range(4)).ravel()}) > 20     # many weight sums
    # colour pitches 3 W + 1 and 3 W + 5, output rows 1 and 3 bytes further apart than packed (the byte path), map pitches that
    # are no multiples of 4, strided grids, windows that cut runs
    _assert_device_equals_numpy(mf, Cur, frames, grids, 64, cut, "pitches + 1", host=bbme, colour_extra=1, out_extra=1, map_extra=1)
    _assert_device_equals_numpy(mf, Cur, frames, grids, 1021, inner, "pitches + 5 / + 3, strided grids", colour_extra=5, out_extra=3,
                                map_extra=3, q_extra=3)
    _assert_device_equals_numpy(mf, Cur, frames, grids, 1, None, "map rows off 8-byte alignment", map_extra=2, q_extra=1)
    wins = odd_windows(CH, CW)
    for n, chosen in enumerate(NEIGHBOUR_SETS[:-1]):       # the other 14 neighbour sets
        _assert_device_equals_numpy(mf, Cur, pick(frames, chosen), pick(grids, chosen), (64, 255, 1021)[n % 3],
                                    (None, cut, inner, wins[3], wins[4])[n % 5], chosen, host=bbme if n % 4 == 0 else None,
                                    colour_extra=(0, 1, 5)[n % 3], out_extra=(0, 1, 3)[(n + 1) % 3], q_extra=3 * (n % 2), map_extra=n % 3)
    _assert_device_equals_numpy(mf, Cur, frames, grids, 255, what="frame only", want=("out",), out_extra=3, q_extra=3)
    _assert_device_equals_numpy(mf, Cur, frames, grids, 1021, what="map only", want=("map",), colour_extra=5, map_extra=1)
    _assert_device_equals_numpy(mf, Cur, frames, grids, 64, cut, "statistics only", want=("stats",), q_extra=3)
    _assert_device_equals_numpy(mf, Cur, frames, grids, 64, inner, "side stream", colour_extra=1, out_extra=1,
                                stream=torch.cuda.Stream())
    # every edge of the padded view: a quarter pel and a pixel out, and all 16 fractions
    Cf, flat = flat_five(w, h, 3 * H0 + W0)
    for n, (Q, cells) in enumerate((edge_grid(H0, W0), edge_fraction_grid(H0, W0))):
        for chosen in ((0, 1, 2, 3), (2,), (1, 3))[:3 - n]:
            exp = _assert_device_equals_numpy(mf, Cf, pick(flat, chosen), pick([Q] * 4, chosen), 1021, None, "edges", colour_extra=1,
                                              out_extra=1, q_extra=3)
            _check_edge_cells(exp, cells, Cf, px, py, chosen)
    x = list(extreme_grids(CH, CW, np.random.default_rng(w)) + extreme_grids(CH, CW, np.random.default_rng(h)))
    for thr in (1, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, Cur, frames, x, thr, what="int16 extremes", colour_extra=1, q_extra=3)
        assert np.array_equal(out, Cur) and not wmap.any() and st == (0,) * 6
    # property 2 in the kernel: neighbours 2 and 3 absent is K13b, bit for bit
    tc, tp, tn, qp, qn = (_cuda(a) for a in (Cur, frames[0], frames[1], grids[0], grids[1]))
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    wmap = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    for thr, win in ((64, cut), (1021, None)):
        mf.cells_temporal_filter_subpel_bgr_device(tc, tp, tn, qp, qn, thr, out=out, weights=wmap, stats=st, window=win)
        mf.synchronize()
        new = _device_filter(mf, Cur, pick(frames, (0, 1)), pick(grids, (0, 1)), thr, win)
        assert np.array_equal(new[0], out.cpu().numpy()) and np.array_equal(new[1], wmap.cpu().numpy().astype(np.uint16))
        assert (new[2][0], new[2][1], new[2][4], new[2][5]) == tuple(st.cpu().tolist()) and new[2][2:4] == (0, 0)
    mf.close()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_division_by_every_weight_sum_in_every_channel_in_the_kernel(bbme, k):
    """Every combination of the four weights, so every S = 8 .. 40 with many numerators, in channel k through the kernel's
    multiply-shift: the 162 x 162 table inside a 164 x 164 frame (the rest is 0 against 0: weight 8)"""
    z = np.zeros((164, 164, 3), np.uint8)
    mf = bbme.MF(z, z, [12], [2])
    assert (mf.padded_height, mf.padded_width, mf.padding_x, mf.padding_y) == (164, 164, 0, 0)

    def embed(a, shape):
        full = np.zeros(shape + a.shape[2:], a.dtype)
        full[:a.shape[0], :a.shape[1]] = a
        return full

    def filt(Cur, frames, grids, thr):
        h, w = Cur.shape[:2]
        out, wmap, st = _assert_device_equals_numpy(mf, embed(Cur, (164, 164)), [embed(f, (164, 164)) for f in frames],
                                                    [embed(g, (82, 82)) for g in grids], thr)
        return out[:h, :w], wmap[:h // 2, :w // 2], st

    weights = weight_sums_in_channel(filt, k)
    assert set((8 + weights.sum(axis=0)).ravel().tolist()) == set(range(8, 41))
    mf.close()


def _guarded_results(bbme):
    """Edge validity and int16 extremes through cells_temporal_filter_wide_bgr_device on a geometry with odd paddings, and the
    own-context calls of a colour chain -> (contexts, sha256 of every result)"""
    w, h, search, block = 130, 98, [12], [4]
    z = np.zeros((h, w, 3), np.uint8)
    mf = bbme.MF(z, z, search, block)
    px, py = mf.padding_x, mf.padding_y
    assert (px, py) == (1, 1)
    H0, W0 = mf.padded_height, mf.padded_width
    CH, CW = mf.cells_shape
    Cur, flat = flat_five(w, h, 5)
    results = []
    for Q, cells in (edge_grid(H0, W0), edge_fraction_grid(H0, W0)):
        for chosen in ((0, 1, 2, 3), (2,), (1, 3)):
            exp = _assert_device_equals_numpy(mf, Cur, pick(flat, chosen), pick([Q] * 4, chosen), 1021, None, "edges", out_extra=1,
                                              colour_extra=1)
            _check_edge_cells(exp, cells, Cur, px, py, chosen)
            results += [exp[0], exp[1], np.array(exp[2])]
    rng = np.random.default_rng(5)
    x = list(extreme_grids(CH, CW, rng) + extreme_grids(CH, CW, rng))
    for thr in (1, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, Cur, flat, x, thr, None, "int16 extremes", q_extra=3)
        assert np.array_equal(out, Cur) and not wmap.any() and st == (0,) * 6
    mf.close()
    frames = [np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))
              for v in bbme.synth_video(130, 98, 5, 5, max_motion=3)]
    chain = bbme.MFChain(frames, search, block)
    chain.estimate_bidirectional_async()
    results += [chain.temporal_filter_run_wide_bgr(96), np.array([_stats(s) for s in chain.temporal_filter_wide_bgr_stats(64, "all")]),
                chain.get_frame_filtered_wide_bgr(2, 64)]
    return [chain], hashlib.sha256(b"".join(np.ascontiguousarray(r).tobytes() for r in results)).hexdigest()


def _guard_child():
    """Runs in a fresh process under BBME_TEST_GUARD=1 and BBME_TEST_POISON=1: prints the digest of the results and the guards' state"""
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    assert os.environ["BBME_TEST_GUARD"] == "1" and os.environ["BBME_TEST_POISON"] == "1"
    ctxs, digest = _guarded_results(bbme)
    live, violations, first = C.c_ulonglong(), C.c_ulonglong(), C.create_string_buffer(512)
    found = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    names = (b"the composed cells of the wide temporal filter", b"the quarter-pel cells of the wide temporal filter",
             b"the colour wide temporal filter statistics")
    for name, f in zip(names, found):
        _capi.check(_capi.lib().bbme_test_guard_find(name, 1, C.byref(f)))
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
    for ctx in ctxs:
        ctx.close()
    after = C.c_ulonglong()
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(after), first, len(first)))
    print("GUARDED %s buffers=%d violations=%d after_close=%d %s" % (digest, sum(bool(f.value) for f in found), violations.value,
                                                                      after.value, first.value.decode()))


def test_edges_and_extremes_under_guard_bands_and_poison(bbme):
    """Validity at every edge and the int16 extremes equal numpy, the valid cells take their neighbours and the others keep C, with
    and without the knobs; the chain's composed and quarter-pel buffers and the colour filter's statistics scratch lie between
    guard bands, and no band is damaged.  The child is a fresh process."""
    ctxs, digest = _guarded_results(bbme)
    for ctx in ctxs:
        ctx.close()
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBME_TEST_GUARD="1", BBME_TEST_POISON="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_wide_temporal_filter_bgr as t; t._guard_child()" % (
        tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:5] == [digest, "buffers=3", "violations=0", "after_close=0"], line[0]


def test_property_1_grey_frames_give_the_grey_wide_filter_of_the_same_context(bbme):
    """B = G = R on a colour chain: every channel of temporal_filter_run_wide_bgr is the unpadded window of
    temporal_filter_run_wide of the SAME context (which filters the luma planes), statistics 0 .. 4 equal, the sixth threefold"""
    w, h, search, block = 130, 98, [12], [4]
    grey = bbme.synth_video(w, h, 5, 300 + w + h, max_motion=3)
    chain = bbme.MFChain([grey3(g) for g in grey], search, block)
    chain.estimate_bidirectional_async()
    px, py = chain.padding_x, chain.padding_y
    assert (px, py) == (1, 1)
    changed = 0
    for thr in (1, 64, 1021):
        plane = chain.temporal_filter_run_wide(thr)[:, py:py + h, px:px + w]
        col = chain.temporal_filter_run_wide_bgr(thr)
        for k in range(3):
            assert np.array_equal(col[..., k], plane), (thr, k)
        changed += int((plane != np.stack(grey)).sum())
        for win in ("all", _odd_window(chain)):
            g = [_stats(s) for s in chain.temporal_filter_wide_stats(thr, win)]
            assert [_stats(s) for s in chain.temporal_filter_wide_bgr_stats(thr, win)] == [s[:5] + (3 * s[5],) for s in g], (thr, win)
    assert changed > 0
    chain.close()


def _luma_fields(bbme, oracle, video):
    """`field(a, b)`: the oracle's integer field on the luma of frame a of the colour video into that of frame b, computed once"""
    search, block = VIDEO_PARAMS
    luma = [np_bgr_to_gray(v) for v in video]
    memo = {}

    def field(a, b):
        if (a, b) not in memo:
            memo[(a, b)] = _oracle_fields(bbme, oracle, luma[a], luma[b], search, block)[1]
        return memo[(a, b)]

    return field


@pytest.fixture(scope="module")
def colour_fields(bbme, oracle):
    """Chains of up to five slots: test_gpu_bgr.colour_video's five 200 x 136 frames; of six: the first six of the seven-frame
    video of the same construction -> {frames: (video, field)}"""
    five, six = colour_video(bbme), _colour7(bbme)[:6]
    return {n: (v, _luma_fields(bbme, oracle, v)) for n, v in ((2, five), (3, five), (5, five), (6, six))}


def _cpu_route(bbme, field, video, f, thr, window=None):
    search, block = VIDEO_PARAMS
    return cpu_wide_bgr_route(bbme, field, video, f, thr, search, block, window)[0]


@pytest.mark.parametrize("n", (5, 6))
def test_chain_equals_the_cpu_route_on_the_oracles_luma_fields(bbme, colour_fields, n):
    search, block = VIDEO_PARAMS
    video, field = colour_fields[n]
    chain = bbme.MFChain(video[:n], search, block)
    chain.estimate_bidirectional_async()
    for p in range(n - 1):
        assert np.array_equal(chain.get_pair_cells(p), field(p, p + 1)) and np.array_equal(chain.get_pair_backward_cells(p), field(p + 1, p))
    win = _odd_window(chain)
    for thr in (64, 1021):
        exp = [_cpu_route(bbme, field, video[:n], f, thr) for f in range(n)]
        run = chain.temporal_filter_run_wide_bgr(thr)                             # every slot from ONE filter launch
        assert run.shape == (n, VIDEO[1], VIDEO[0], 3)
        for f in range(n):
            assert np.array_equal(run[f], exp[f][0]), (thr, f)
            assert np.array_equal(chain.get_frame_filtered_wide_bgr(f, thr), exp[f][0]), (thr, f)   # a run equals its frames one by one
        assert np.array_equal(chain.temporal_filter_run_wide_bgr(thr, 1, n - 2), run[1:n - 1])
        assert np.array_equal(chain.temporal_filter_run_wide_bgr(thr, 2, 1)[0], run[2])
        assert np.array_equal(chain.temporal_filter_run_wide_bgr(thr, n - 2, 2), run[n - 2:])
        assert [_stats(s) for s in chain.temporal_filter_wide_bgr_stats(thr, "all")] == [e[2] for e in exp], thr
    assert [_stats(s) for s in chain.temporal_filter_wide_bgr_stats(64, win)] == \
        [_cpu_route(bbme, field, video[:n], f, 64, win)[2] for f in range(n)]
    mid = _cpu_route(bbme, field, video[:n], 2, 64)[2]
    assert all(mid[k] > 0 for k in range(4))               # the middle slot takes from all four neighbours
    chain.close()


@pytest.mark.parametrize("n", (2, 3))
def test_short_chains_degrade_as_the_rule_says(bbme, colour_fields, n):
    """Two slots: each has one neighbour at distance 1; three: the middle one two, the ends one at distance 1 and one at 2"""
    search, block = VIDEO_PARAMS
    video, field = colour_fields[n]
    chain = bbme.MFChain(video[:n], search, block)
    chain.estimate_bidirectional_async()
    exp = [_cpu_route(bbme, field, video[:n], f, 96) for f in range(n)]
    run = chain.temporal_filter_run_wide_bgr(96)
    stats = chain.temporal_filter_wide_bgr_stats(96, "all")
    for f in range(n):
        assert np.array_equal(run[f], exp[f][0]) and _stats(stats[f]) == exp[f][2], f
    present = [[_stats(s)[k] > 0 for k in range(4)] for s in stats]
    assert present == ([[False, True, False, False], [True, False, False, False]] if n == 2 else
                       [[False, True, False, True], [True, True, False, False], [True, False, True, False]])
    if n == 2:                                             # property 2: neighbours 2 and 3 missing is the colour subpel filter
        assert np.array_equal(run, chain.temporal_filter_run_subpel_bgr(96))
        sub = chain.temporal_filter_subpel_bgr_stats(96, "all")
        assert [(s[0], s[1], s[4], s[5]) for s in map(_stats, stats)] == [tuple(d[k] for k in STAT_KEYS) for d in sub]
    chain.close()


def test_needs_fields_and_stored_colour(bbme):
    from blockbasedmotionestimation_amd import _capi
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    state = _capi.ERR_STATE
    mf = bbme.MFChain(video, search, block)
    calls = (lambda: mf.temporal_filter_run_wide_bgr(64), lambda: mf.get_frame_filtered_wide_bgr(2, 64),
             lambda: mf.temporal_filter_wide_bgr_stats(64))
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # no bidirectional estimate yet
    mf.estimate_async()
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # a forward estimate is none either
    mf.estimate_bidirectional_async()
    run, stats = mf.temporal_filter_run_wide_bgr(64), mf.temporal_filter_wide_bgr_stats(64)
    grey = mf.temporal_filter_run_wide(64)
    mf.set_frame_run(4, [np_bgr_to_gray(video[4])])        # a grey setter withdraws slot 4's colour
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # and the fields
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter_run_wide(64), grey)                   # the same luma: the grey filter stands
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # slot 2 reads slot 4
    assert _status(bbme, lambda: mf.temporal_filter_run_wide_bgr(64, 3, 1)) == state
    assert np.array_equal(mf.temporal_filter_run_wide_bgr(64, 0, 2), run[:2])      # slots 0 and 1 read slots 0 .. 3 only
    assert np.array_equal(mf.get_frame_filtered_wide_bgr(1, 64), run[1])
    mf.set_frame_run(4, [video[4]])
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # colour again, but no fields
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter_run_wide_bgr(64), run) and mf.temporal_filter_wide_bgr_stats(64) == stats
    mf.close()


def test_changes_no_state_and_refuses_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    inv, unsupported = _capi.ERR_INVALID, _capi.ERR_UNSUPPORTED
    mf = bbme.MFChain(video, search, block)
    mf.estimate_bidirectional_async()
    h, w = VIDEO[1], VIDEO[0]
    CH, CW = mf.cells_shape

    def state():
        return dict(cells=[mf.get_pair_cells(p) for p in range(4)], back=[mf.get_pair_backward_cells(p) for p in range(4)],
                    planes=[mf.get_slot_plane(l, s) for l in range(3) for s in range(5)],
                    colour=[mf.frame_bgr_tensor(0, 0).cpu().numpy()] + [mf.frame_bgr_tensor(p, 1).cpu().numpy() for p in range(4)],
                    flow=mf.get_pair_flow(1), grey=mf.temporal_filter_run_wide(64), near=mf.temporal_filter_run_subpel_bgr(64))

    def digest(s):
        return {k: [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in (v if isinstance(v, list) else [v])]
                for k, v in s.items()}

    before = digest(state())
    run = mf.temporal_filter_run_wide_bgr(64)
    stats = mf.temporal_filter_wide_bgr_stats(64, "all")
    # the cells call on the context's own colour and the grids the run used gives the run's frame and statistics
    colour = [mf.frame_bgr_tensor(0, 0).clone()] + [mf.frame_bgr_tensor(p, 1).clone() for p in range(4)]
    planes = [mf.get_slot_plane(0, s) for s in range(5)]
    q = [torch.from_numpy(bbme.subpel_cells(planes[2], planes[n], g)[0]).cuda()
         for n, g in ((1, mf.get_pair_backward_cells(1)), (3, mf.get_pair_cells(2)), (0, mf.composed_cells(2, -1)), (4, mf.composed_cells(2, 1)))]
    out = torch.zeros((5, h, w, 3), dtype=torch.uint8, device="cuda")
    wmap = torch.zeros((CH, CW), dtype=torch.int16, device="cuda")
    st = torch.zeros(6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    nb = [colour[1], colour[3], colour[0], colour[4]]
    mf.cells_temporal_filter_wide_bgr_device(colour[2], nb, q, 64, out=out[0], weights=wmap, stats=st)
    mf.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), run[2]) and tuple(st.cpu().tolist()) == _stats(stats[2])
    # the grey wide calls share the quarter-pel buffers, the subpel calls the +-1 buffer: the next colour run makes its grids again
    mf.temporal_filter_wide_stats(64, "all")
    mf.temporal_filter_run_subpel_bgr(64)
    assert np.array_equal(mf.temporal_filter_run_wide_bgr(64), run) and mf.temporal_filter_wide_bgr_stats(64, "all") == stats
    assert digest(state()) == before
    # argument errors
    ctx = mf._ctx
    four = lambda ts: (C.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in ts])      # noqa: E731
    c_, o_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (colour[2], out, wmap, st))
    buf = np.zeros((h, w, 3), np.uint8)
    s30 = (C.c_ulonglong * 30)()

    def cells(f=nb, c=c_, bp=3 * w, g=q, qpitch=CW, thr=64, win=None, o=o_, op=3 * w, m=m_, mp=CW, s=s_):
        return L.bbme_cells_wide_temporal_filter_bgr_device(ctx, four(f), c, bp, four(g), qpitch, thr, win, o, op, m, mp, s, None)

    def run_of(first=0, count=5, thr=64, o=o_, op=3 * w, os=3 * h * w):
        return L.bbme_wide_temporal_filter_bgr_chain_device(ctx, first, count, thr, o, op, os, None)

    def host(slot=0, thr=64, o=buf.ctypes.data):
        return L.bbme_get_wide_temporal_filtered_bgr_host(ctx, slot, thr, o)

    assert cells() == 0 and run_of() == 0 and host() == 0
    for k in range(4):
        assert cells(f=pick(nb, (k,)), g=pick(q, (k,))) == 0                         # each neighbour alone
        assert cells(f=pick(nb, (k,))) == inv and cells(g=pick(q, (k,))) == inv      # a frame without its grid, ...
    assert cells(f=[None] * 4, g=[None] * 4) == inv and cells(c=None) == inv
    assert cells(o=None, m=None, s=None) == inv                                     # nothing asked for
    assert cells(o=None) == 0 and cells(m=None) == 0 and cells(s=None) == 0 and cells(o=None, m=None) == 0
    assert cells(qpitch=CW - 1) == inv and cells(qpitch=0) == inv
    assert cells(bp=3 * w - 1) == inv and cells(op=3 * w - 1) == inv and cells(mp=CW - 1) == inv
    assert cells(mp=CW - 1, m=None) == 0 and cells(op=3 * w - 1, o=None) == 0       # a pitch of nothing is not looked at
    for frame in [colour[2]] + nb:                                                  # an output inside an input frame
        assert cells(o=C.c_void_p(frame.data_ptr())) == inv
    assert cells(o=C.c_void_p(c_.value + 3 * w)) == inv
    assert cells(f=pick(nb, (0,)), g=pick(q, (0,)), o=C.c_void_p(nb[1].data_ptr())) == 0      # an absent neighbour is no input
    assert run_of(o=None) == inv and host(o=None) == inv
    assert L.bbme_wide_temporal_filter_bgr_stats(ctx, 64, None, None) == inv
    for thr in (0, -5, 1022):
        assert cells(thr=thr) == inv and run_of(thr=thr) == inv and host(thr=thr) == inv, thr
        assert L.bbme_wide_temporal_filter_bgr_stats(ctx, thr, None, s30) == inv
    for slot in (-1, 5):
        assert host(slot=slot) == inv
    for first, count in ((-1, 1), (0, 0), (0, 6), (5, 1), (4, 2), (1, -1)):
        assert run_of(first=first, count=count) == inv, (first, count)
    assert run_of(first=4, count=1) == 0 and run_of(first=1, count=3) == 0
    assert run_of(op=3 * w - 1) == inv and run_of(count=2, os=3 * h * w - 1) == inv
    assert run_of(count=1, os=0) == 0                                               # one frame has no stride
    for win in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (CW - 7, 0, 8, 8), (0, CH - 7, 8, 8), (0, 0, CW + 1, CH)):
        w4 = (C.c_int * 4)(*win)
        assert cells(win=w4) == inv, win
        assert L.bbme_wide_temporal_filter_bgr_stats(ctx, 64, w4, s30) == inv, win
    assert L.bbme_wide_temporal_filter_bgr_stats(ctx, 64, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s30) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.temporal_filter_run_wide_bgr(64, 3, 3)
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_wide_bgr_device(colour[2], nb, [q[0][:, :CW - 2]] + q[1:], 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_wide_bgr_device(colour[2], [nb[0][:, :w - 1]] + nb[1:], q, 64, out=out[0])
    assert e.value.status == inv
    mf.synchronize()
    assert digest(state()) == before and np.array_equal(mf.temporal_filter_run_wide_bgr(64), run)
    mf.close()
    # a pair or batched context has no chain of slots: BBME_ERR_UNSUPPORTED; the cells call needs no chain
    for other in (bbme.MF(video[0], video[1], search, block), bbme.MFBatch([(video[0], video[1]), (video[1], video[2])], search, block)):
        other.estimate_bidirectional_async()
        ctx = other._ctx
        assert run_of(count=1) == unsupported and host() == unsupported
        assert L.bbme_wide_temporal_filter_bgr_stats(ctx, 64, None, s30) == unsupported
        z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
        cur = torch.full((h, w, 3), 9, dtype=torch.uint8, device="cuda")
        res = torch.zeros_like(cur)
        other.cells_temporal_filter_wide_bgr_device(cur, [None, None, cur, None], [None, None, z, None], 64, out=res)
        other.synchronize()
        assert bool((res == 9).all())
        other.close()


@pytest.fixture(scope="module")
def denoise_video(bbme, oracle):
    """Seven 200 x 136 colour frames and, per frame, the CPU route on the oracle's luma fields, every neighbour that exists"""
    video = _colour7(bbme)
    field = _luma_fields(bbme, oracle, video)
    return video, [_cpu_route(bbme, field, video, f, 96)[0] for f in range(len(video))]


@pytest.mark.parametrize("window", (1, 3, 8))
def test_denoise_frames_wide_in_colour(bbme, denoise_video, window):
    """window = 8: one run, one chain of seven frames; window = 3: runs on chains of five, seven and three frames; window = 1: a
    chain per frame, of three, four, five, ... frames: every frame still filtered from every neighbour the video has"""
    from blockbasedmotionestimation_amd import _capi
    from blockbasedmotionestimation_amd.sequence import denoise_frames_wide
    search, block = VIDEO_PARAMS
    video, exp = denoise_video
    keep = [v.copy() for v in video]
    got = denoise_frames_wide(video, search, block, 96, window=window, bgr=True)
    assert len(got) == len(video)
    for v, k in zip(video, keep):
        assert np.array_equal(v, k)
    for f in range(len(video)):
        assert got[f].shape == (VIDEO[1], VIDEO[0], 3) and got[f].dtype == np.uint8
        assert np.array_equal(got[f], exp[f]), f
    assert any(not np.array_equal(got[f], video[f]) for f in range(len(video)))
    if window == 8:
        with pytest.raises(bbme.BbmeError) as e:           # without the keyword a colour video is refused as before
            denoise_frames_wide(video[:3], search, block, 96)
        assert e.value.status == _capi.ERR_UNSUPPORTED and "grey" in e.value.message
        with pytest.raises(ValueError):
            denoise_frames_wide([np_bgr_to_gray(v) for v in video[:3]], search, block, 96, bgr=True)
