"""Temporal filtering of colour frames along quarter-pel grids on the GPU (include/bbme.h, "BGR SUBPEL TEMPORAL FILTER RULE"), all
bit-exact through the C-ABI: k_subpel_temporal_filter_bgr gives the numpy restatement of tests/test_subpel_temporal_filter_bgr_cpu.py
and the host rule on a caller's frames and grids -- every fraction at every edge of the padded view, geometries with odd paddings
and cut runs, colour and output pitches that reach the byte paths, strided grids and maps, odd windows, a side stream, each output
alone -- and on the stored colour with the context's own refined fields; grey frames give k_subpel_temporal_filter's bytes in
every channel and 4 x integer grids k_temporal_filter_bgr's; both divisions are exact in every channel, on frame bytes and on
sampled costs; chains filter every slot from both sides, batches from one; guard bands stay intact; the calls need fields and stored
colour, change no context state and refuse bad arguments; sequence.denoise_frames(subpel_bgr=True) and bbme_cli --denoise-subpel
produce the same colour frames."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _cuda, _odd_window, _stats_of, _status
from test_bgr_cpu import SHAPES, np_bgr_to_gray
from test_gpu_bgr import VIDEO, VIDEO_PARAMS, _write_ppm, colour_video
from test_gpu_bidirectional import CASES, _frames, _oracle_fields
from test_gpu_temporal_filter_bgr import _colour7, _pitched_tensor, _video_fields
from test_interpolation_cpu import extreme_grids, odd_windows
from test_subpel_interpolation_cpu import fraction_grids
from test_subpel_temporal_filter_bgr_cpu import (division_tables_in_channel, edge_fraction_grid, flat_triple, near_smooth_triple,
                                                 np_subpel_temporal_filter_bgr, sampled_costs_in_channel, times4)
from test_subpel_temporal_filter_cpu import edge_grid
from test_temporal_filter_bgr_cpu import near_colour_triple, near_grids
from test_temporal_filter_cpu import RULE_THRS, STAT_KEYS, neighbour_sets

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

_cache = {}

WHOLE_RUNS = (200, 136, (30, 30, 30), (16, 16, 16))        # pads to 256 x 192: whole runs, even paddings (28, 28)
GEOMETRIES = dict(SHAPES)
GEOMETRIES[WHOLE_RUNS] = (256, 192, 28, 28)


def _device_filter(mf, Cur, P, QP, N, QN, thr, window=None, colour_extra=0, out_extra=0, q_extra=0, map_extra=0, stream=None,
                   want=("out", "map", "stats"), integer=False):
    """cells_temporal_filter_subpel_bgr_device (integer: cells_temporal_filter_bgr_device) on host frames and grids -> (frame
    (H, W, 3), map (CH, CW), stats tuple), None where not asked for.  The colour frames' rows are colour_extra bytes, the output's
    rows out_extra bytes, the map's rows map_extra bytes and both grids' rows q_extra cells further apart than packed; the bytes
    and cells in between and the 64 bytes behind the frame's last row stay untouched."""
    import torch
    CH, CW = mf.cells_shape
    h, w = mf.orig_height, mf.orig_width
    tc, tp, tn = (_pitched_tensor(a, colour_extra) for a in (Cur, P, N))
    grids = []
    for Q in (QP, QN):
        if Q is None:
            grids.append(None)
            continue
        t = torch.full((CH, CW + q_extra, 2), 0x7777, dtype=torch.int16, device="cuda")
        t[:, :CW] = _cuda(np.asarray(Q, np.int16))
        grids.append(t)
    pitch = 3 * w + out_extra
    raw = torch.full((h * pitch + 64,), 0xAA, dtype=torch.uint8, device="cuda") if "out" in want else None
    out = None if raw is None else raw.as_strided((h, w, 3), (pitch, 3, 1))
    wmap = torch.full((CH, CW + map_extra), 0xAA, dtype=torch.uint8, device="cuda") if "map" in want else None
    st = torch.zeros(4, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    views = [None if t is None else (t[:, :CW] if q_extra else t[:, :CW].contiguous()) for t in grids]
    kw = dict(out=out, weights=None if wmap is None else wmap[:, :CW], stats=st, window=window)
    handle = None if stream is None else stream.cuda_stream
    if integer:
        mf.cells_temporal_filter_bgr_device(tc, tp, tn, views[0], views[1], thr, hip_stream_handle=handle, **kw)
    else:
        mf.cells_temporal_filter_subpel_bgr_device(tc, tp, tn, views[0], views[1], thr, stream=handle, **kw)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    if raw is not None:
        rows = raw[:h * pitch].view(h, pitch)
        assert bool((rows[:, 3 * w:] == 0xAA).all()) and bool((raw[h * pitch - out_extra:] == 0xAA).all())
    assert wmap is None or not map_extra or bool((wmap[:, CW:] == 0xAA).all())
    for t in grids:
        assert t is None or bool((t[:, CW:] == 0x7777).all())
    return (None if out is None else out.cpu().numpy(), None if wmap is None else wmap[:, :CW].cpu().numpy(),
            None if st is None else tuple(st.cpu().tolist()))


def _host(bbme, Cur, P, QP, N, QN, thr, px, py, window=None):
    out, wmap, st = bbme.temporal_filter_cells_subpel_bgr(Cur, P, N, QP, QN, thr, px, py, window)
    return out, wmap, _stats(st)


def _assert_device_equals_numpy(mf, Cur, P, QP, N, QN, thr, window=None, what=None, host=None, **kw):
    """GPU = numpy (= the host rule where `host` is the package)"""
    out, wmap, st = _device_filter(mf, Cur, P, QP, N, QN, thr, window, **kw)
    px, py = mf.padding_x, mf.padding_y
    exp = np_subpel_temporal_filter_bgr(Cur, P, QP, N, QN, thr, px, py, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert out is None or np.array_equal(out, exp[0]), tag
    assert wmap is None or np.array_equal(wmap, exp[1]), tag
    assert st is None or st == exp[2], tag
    if host is not None:
        h = _host(host, Cur, P, QP, N, QN, thr, px, py, window)
        assert np.array_equal(h[0], exp[0]) and np.array_equal(h[1], exp[1]) and h[2] == exp[2], tag
    return exp


def _check_edge_cells(exp, cells, Cur, px, py, p, q):
    """The valid cells took their neighbour; the others have weight 0 and keep C's pixels"""
    out, wmap = exp[:2]
    full, padC = (np.pad(f, ((py, py), (px, px), (0, 0))) for f in (out, Cur))
    for cx, cy, valid in cells:
        wp, wn = wmap[cy, cx] & 0x0f, wmap[cy, cx] >> 4
        assert (wp > 0) == (valid and p is not None) and (wn > 0) == (valid and q is not None), (cx, cy, valid)
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
    wins = odd_windows(CH, CW)
    # every fraction on smooth frames: both neighbours and each alone, strengths, windows, colour pitches 3 W + 1 and 3 W + 5,
    # output rows 0, 1 and 3 bytes further apart than packed (the dword path and the byte path), strided grids and maps
    Cur, P, N = near_smooth_triple(w, h, 10 * h + w)
    qp, qn = fraction_grids(H0, W0, 100 * W0 + H0)
    every = {(a, b) for a in range(4) for b in range(4)}
    for n, thr in enumerate(RULE_THRS):
        for k, (p, a, q, b) in enumerate(neighbour_sets(P, qp, N, qn)):
            exp = _assert_device_equals_numpy(mf, Cur, p, a, q, b, thr, wins[(n + k) % len(wins)], shape, host=bbme,
                                              colour_extra=(0, 1, 5)[(n + k) % 3], out_extra=(0, 1, 3)[(n + 2 * k) % 3],
                                              q_extra=(0, 3)[(n + k) % 2], map_extra=(1, 0)[(n + k) % 2])
            if thr == 1021 and k == 0:
                for wbits, Q in ((exp[1] & 0x0f, qp), (exp[1] >> 4, qn)):             # every fraction class was taken, by both
                    assert {(int(u) & 3, int(v) & 3) for u, v in Q[wbits > 0]} == every
    # all 16 fractions at every edge of the padded view, and the grey test's edge grid (a quarter pel and a pixel out)
    Cf, Pf, Nf = flat_triple(w, h, 3 * H0 + W0)
    for Q, cells in (edge_fraction_grid(H0, W0), edge_grid(H0, W0)):
        for p, a, q, b in neighbour_sets(Pf, Q, Nf, Q):
            exp = _assert_device_equals_numpy(mf, Cf, p, a, q, b, 1021, None, "edges", host=bbme, colour_extra=1, out_extra=1, q_extra=3)
            _check_edge_cells(exp, cells, Cf, px, py, p, q)
    # random frames, far vectors, a side stream, each output alone
    Cr, Pr, Nr = near_colour_triple(w, h, 7 * w + h)
    fp, fn = fraction_grids(H0, W0, 3 * W0 + H0, reach=5)
    _assert_device_equals_numpy(mf, Cr, Pr, fp, Nr, fn, 255, wins[1], "side stream", colour_extra=1, out_extra=1, map_extra=1,
                                stream=torch.cuda.Stream())
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 255, what="frame only", want=("out",), out_extra=3, q_extra=3)
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 1021, what="map only", want=("map",), colour_extra=5, map_extra=1)
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 64, wins[3], "statistics only", want=("stats",), q_extra=3)
    ep, en = extreme_grids(CH, CW, np.random.default_rng(w))
    for thr in (1, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, Cr, Pr, ep, Nr, en, thr, what="int16 extremes", colour_extra=1, q_extra=3)
        assert np.array_equal(out, Cr) and not wmap.any() and st == (0, 0, 0, 0)
    # property 2 in the kernel: 4 x integer grids through K13b are K9b on the grids
    gp, gn = near_grids(CH, CW, np.random.default_rng(3 * w + h))
    for thr, win in ((64, wins[3]), (1021, None)):
        old = _device_filter(mf, Cr, Pr, gp, Nr, gn, thr, win, integer=True, colour_extra=1)
        new = _device_filter(mf, Cr, Pr, times4(gp), Nr, times4(gn), thr, win, colour_extra=1, q_extra=3)
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]) and old[2] == new[2], thr
    mf.close()


def _colour_of(v):
    """Three different pointwise maps of a grey frame, as test_gpu_bgr.colour_video's"""
    return np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))


@pytest.mark.parametrize("name", ["cfg1_like", "border_motion"])
def test_the_contexts_own_on_the_oracles_refined_fields(bbme, oracle, name):
    _, _, search, block, _, _, _ = CASES[name]
    c1, c2 = (_colour_of(f) for f in _frames(bbme, name))
    y1, y2 = np_bgr_to_gray(c1), np_bgr_to_gray(c2)
    _, fwd = _oracle_fields(bbme, oracle, y1, y2, search, block, key=(name, "bgr luma", "f"))
    _, bwd = _oracle_fields(bbme, oracle, y2, y1, search, block, key=(name, "bgr luma", "b"))
    mf = bbme.MF(c1, c2, search, block)
    mf.estimate_bidirectional_async()
    px, py = mf.padding_x, mf.padding_y
    I1, I2 = mf.get_level_planes(0)
    assert np.array_equal(I1, bbme.pad_zero(y1, px, py)) and np.array_equal(mf.get_cells(), fwd) and np.array_equal(mf.get_backward_cells(), bwd)
    qf, qb = bbme.subpel_cells(I1, I2, fwd)[0], bbme.subpel_cells(I2, I1, bwd)[0]
    assert np.array_equal(mf.subpel_cells("forward"), qf) and np.array_equal(mf.subpel_cells("backward"), qb)
    assert (qf & 3).any() and (qb & 3).any()
    odd = _odd_window(mf)
    own = [(c1, None, None, c2, qf), (c2, c1, qb, None, None)]
    for thr in (1, 64, 1021):
        for which in (0, 1):
            assert np.array_equal(mf.temporal_filter_subpel_bgr(thr, which), np_subpel_temporal_filter_bgr(*own[which], thr, px, py)[0]), (thr, which)
        for win, np_win in ((None, mf.default_cell_window()), ("all", None), (odd, odd)):
            got = mf.temporal_filter_subpel_bgr_stats(thr, win)
            assert [_stats(g) for g in got] == [np_subpel_temporal_filter_bgr(*own[k], thr, px, py, np_win)[2] for k in (0, 1)], (thr, win)
    # the same through the entry point that takes any frames and grids; injected calls leave the context's own alone
    _assert_device_equals_numpy(mf, *own[0], 64, what="image 1, refined grid")
    _assert_device_equals_numpy(mf, *own[1], 64, odd, "image 2, refined grid", q_extra=3, colour_extra=1)
    _assert_device_equals_numpy(mf, c2, c1, qb, c1, qb, 64, odd, "image 2 between two copies of image 1", out_extra=3, map_extra=1)
    assert np.array_equal(mf.temporal_filter_subpel_bgr(64), np_subpel_temporal_filter_bgr(*own[0], 64, px, py)[0])
    assert np.array_equal(mf.temporal_filter_subpel_bgr(64, 1), np_subpel_temporal_filter_bgr(*own[1], 64, px, py)[0])
    mf.close()


@pytest.mark.parametrize("shape", [s for s in SHAPES][:3:2] + [WHOLE_RUNS])
def test_property_1_grey_frames_give_the_grey_subpel_filter_of_the_same_context(bbme, shape):
    w, h, search, block = shape
    _, _, px, py = GEOMETRIES[shape]
    g1, g2, _ = bbme.synth_pair(w, h, 300 + w + h, max_motion=3)
    mf = bbme.MF(np.repeat(g1[..., None], 3, 2), np.repeat(g2[..., None], 3, 2), list(search), list(block))
    mf.estimate_bidirectional_async()
    CH, CW = mf.cells_shape
    changed = 0
    for thr in RULE_THRS:
        for which in (0, 1):
            grey = mf.temporal_filter_subpel(thr, which)[py:py + h, px:px + w]
            col = mf.temporal_filter_subpel_bgr(thr, which)
            for k in range(3):
                assert np.array_equal(col[..., k], grey), (thr, which, k)
            changed += int((grey != (g1, g2)[which]).sum())
        for win in (None, "all", odd_windows(CH, CW)[1]):
            grey = [_stats(s) for s in mf.temporal_filter_subpel_stats(thr, win)]
            assert [_stats(s) for s in mf.temporal_filter_subpel_bgr_stats(thr, win)] == [(a, b, c, 3 * d) for a, b, c, d in grey], (thr, win)
    assert changed > 0
    # property 2 on the context's own: 4 x the integer cells through the grid call are temporal_filter_bgr
    c1, c2 = np.repeat(g1[..., None], 3, 2), np.repeat(g2[..., None], 3, 2)
    new = _device_filter(mf, c1, None, None, c2, times4(mf.get_cells()), 64)
    assert np.array_equal(new[0], mf.temporal_filter_bgr(64, 0))
    mf.close()


@pytest.fixture(scope="module")
def table_contexts(bbme):
    """One-level contexts without padding of the sizes of the division tables (92 x 92, 132 x 100) and of the sampled-cost table
    (128 x 64): the tables are injected as tensors."""
    ctxs = {}
    for w, h in ((92, 92), (132, 100), (128, 64)):
        z = np.zeros((h, w, 3), np.uint8)
        ctxs[(h, w)] = bbme.MF(z, z, [12], [2])
        assert (ctxs[(h, w)].padded_width, ctxs[(h, w)].padded_height) == (w, h)
    yield ctxs
    for mf in ctxs.values():
        mf.close()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_divisions_are_exact_in_every_channel_in_the_kernel(table_contexts, k):
    def filt(Cur, P, QP, N, QN, thr):
        return _device_filter(table_contexts[Cur.shape[:2]], Cur, P, QP, N, QN, thr)

    division_tables_in_channel(filt, k)
    for thr in (1, 64, 1021):
        sampled_costs_in_channel(filt, k, thr)


def _video_reference(bbme, key, video):
    """Per pair of the colour video the single contexts' integer fields (test_gpu_temporal_filter_bgr._video_fields) refined on the
    CPU on the padded luma planes -> (quarter-pel forward grids, backward grids, (px, py))"""
    if key not in _cache:
        fwd, bwd, (px, py) = _video_fields(bbme, key, video)
        planes = [bbme.pad_zero(np_bgr_to_gray(v), px, py) for v in video]
        _cache[key] = ([bbme.subpel_cells(planes[p], planes[p + 1], fwd[p])[0] for p in range(len(video) - 1)],
                       [bbme.subpel_cells(planes[p + 1], planes[p], bwd[p])[0] for p in range(len(video) - 1)], (px, py))
    return _cache[key]


def _video_rule(video, ref, f, thr, window=None, side=None):
    """The rule on frame f of the video with the refined fields: both neighbours where they exist, or one `side`."""
    qf, qb, (px, py) = ref
    last = len(video) - 1
    prev = f > 0 and side in (None, "prev")
    nxt = f < last and side in (None, "next")
    return np_subpel_temporal_filter_bgr(video[f], video[f - 1] if prev else None, qb[f - 1] if prev else None,
                                         video[f + 1] if nxt else None, qf[f] if nxt else None, thr, px, py, window)


def test_chain_filters_every_slot_and_batch_one_side(bbme):
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)[:4]
    ref = _video_reference(bbme, "chain4", video)
    chain = bbme.MFChain(video, search, block)
    chain.estimate_bidirectional_async()
    for p in range(3):
        assert np.array_equal(chain.get_pair_subpel_cells(p, "forward"), ref[0][p])
        assert np.array_equal(chain.get_pair_subpel_cells(p, "backward"), ref[1][p])
    CH, CW = chain.cells_shape
    win = odd_windows(CH, CW)[1]
    for thr in (64, 1021):
        exp = [_video_rule(video, ref, f, thr)[0] for f in range(4)]
        run = chain.temporal_filter_run_subpel_bgr(thr)                          # every slot from ONE launch
        assert run.shape == (4, VIDEO[1], VIDEO[0], 3)
        for f in range(4):
            assert np.array_equal(run[f], exp[f]), (thr, f)
        assert np.array_equal(chain.temporal_filter_run_subpel_bgr(thr, 1, 2), np.stack(exp[1:3]))
        assert np.array_equal(chain.temporal_filter_run_subpel_bgr(thr, 3, 1)[0], exp[3])
        assert np.array_equal(chain.temporal_filter_run_subpel_bgr(thr, 0, 1)[0], exp[0])
        for p in range(3):                                                       # the slots one by one
            assert np.array_equal(chain.get_frame_filtered_subpel_bgr(p, 0, thr), exp[p]), (thr, p)
            assert np.array_equal(chain.get_frame_filtered_subpel_bgr(p, 1, thr), exp[p + 1]), (thr, p)   # (p, 1) and (p + 1, 0): one frame
        assert np.array_equal(chain.temporal_filter_subpel_bgr(thr), exp[0])
        for w, np_win in ((None, chain.default_cell_window()), ("all", None), (win, win)):
            assert [_stats(s) for s in chain.temporal_filter_subpel_bgr_stats(thr, w)] == \
                [_video_rule(video, ref, f, thr, np_win)[2] for f in range(4)], (thr, w)
    inner = _video_rule(video, ref, 1, 64)
    assert (inner[1] & 0x0f).any() and (inner[1] >> 4).any()                       # inner frames take from both sides
    chain.close()
    # a batch of the same pairs: every frame one-sided
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(3)], search, block)
    batch.estimate_bidirectional_async()
    for p in (2, 0, 1):
        assert np.array_equal(batch.get_frame_filtered_subpel_bgr(p, 0, 64), _video_rule(video, ref, p, 64, side="next")[0]), p
        assert np.array_equal(batch.get_frame_filtered_subpel_bgr(p, 1, 64), _video_rule(video, ref, p + 1, 64, side="prev")[0]), p
    for w, np_win in ((win, win), ("all", None)):
        exp = []
        for p in range(3):
            exp += [_video_rule(video, ref, p, 64, np_win, side="next")[2], _video_rule(video, ref, p + 1, 64, np_win, side="prev")[2]]
        assert [_stats(s) for s in batch.temporal_filter_subpel_bgr_stats(64, w)] == exp, w
    batch.close()


def _guarded_results(bbme):
    """Edge validity and int16 extremes through cells_temporal_filter_subpel_bgr_device on a geometry with odd paddings, and the
    own-context calls of a single and a chain context -> (contexts, sha256 of every result)"""
    w, h, search, block = 130, 98, [12], [4]
    z = np.zeros((h, w, 3), np.uint8)
    mf = bbme.MF(z, z, search, block)
    px, py = mf.padding_x, mf.padding_y
    assert (px, py) == (1, 1)
    H0, W0 = mf.padded_height, mf.padded_width
    Cur, P, N = flat_triple(w, h, 5)
    results = []
    for Q, cells in (edge_grid(H0, W0), edge_fraction_grid(H0, W0)):
        for p, a, q, b in ((P, Q, N, Q), (P, Q, None, None), (None, None, N, Q)):
            exp = _assert_device_equals_numpy(mf, Cur, p, a, q, b, 1021, None, "edges", out_extra=1, colour_extra=1)
            _check_edge_cells(exp, cells, Cur, px, py, p, q)
            results += [exp[0], exp[1], np.array(exp[2])]
    rng = np.random.default_rng(5)
    xp, xn = extreme_grids(H0 // 2, W0 // 2, rng)
    for thr in (1, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, Cur, P, xp, N, xn, thr, None, "int16 extremes", q_extra=3)
        assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)
    mf.close()
    frames = [_colour_of(v) for v in bbme.synth_video(130, 98, 3, 5, max_motion=3)]
    single = bbme.MF(frames[0], frames[1], search, block)
    chain = bbme.MFChain(frames, search, block)
    for ctx in (single, chain):
        ctx.estimate_bidirectional_async()
    results += [single.temporal_filter_subpel_bgr(64, 0), single.temporal_filter_subpel_bgr(64, 1), chain.temporal_filter_run_subpel_bgr(96)]
    results += [np.array([_stats(s) for s in ctx.temporal_filter_subpel_bgr_stats(64, "all")]) for ctx in (single, chain)]
    return [single, chain], hashlib.sha256(b"".join(np.ascontiguousarray(r).tobytes() for r in results)).hexdigest()


def _guard_child():
    """Runs in a fresh process under BBME_TEST_GUARD=1 and BBME_TEST_POISON=1: prints the digest of the results and the guards' state"""
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    assert os.environ["BBME_TEST_GUARD"] == "1" and os.environ["BBME_TEST_POISON"] == "1"
    ctxs, digest = _guarded_results(bbme)
    live, violations, first = C.c_ulonglong(), C.c_ulonglong(), C.create_string_buffer(512)
    found = C.c_void_p()
    _capi.check(_capi.lib().bbme_test_guard_find(b"the quarter-pel cells of the temporal filter", 1, C.byref(found)))
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
    for ctx in ctxs:
        ctx.close()
    after = C.c_ulonglong()
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(after), first, len(first)))
    print("GUARDED %s buffer=%d violations=%d after_close=%d %s" % (digest, bool(found.value), violations.value, after.value,
                                                                     first.value.decode()))


def test_edges_and_extremes_under_guard_bands_and_poison(bbme):
    """Validity at every edge and the int16 extremes equal numpy, the valid cells take their neighbour and the others keep C, with
    and without the knobs; the context's quarter-pel buffer and statistics scratch lie between guard bands, and no band is
    damaged."""
    ctxs, digest = _guarded_results(bbme)
    for ctx in ctxs:
        ctx.close()
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBME_TEST_GUARD="1", BBME_TEST_POISON="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_subpel_temporal_filter_bgr as t; t._guard_child()" % (
        tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:5] == [digest, "buffer=1", "violations=0", "after_close=0"], line[0]


def test_needs_fields_and_stored_colour(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    c1, c2 = video[:2]
    g1, g2 = np_bgr_to_gray(c1), np_bgr_to_gray(c2)
    state = _capi.ERR_STATE
    h, w = VIDEO[1], VIDEO[0]
    mf = bbme.MF(c1, c2, search, block)
    calls = (lambda: mf.temporal_filter_subpel_bgr(64), lambda: mf.temporal_filter_subpel_bgr(64, 1),
             lambda: mf.temporal_filter_subpel_bgr_stats(64))
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # no bidirectional estimate yet
    out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    op = C.c_void_p(out.data_ptr())
    assert L.bbme_subpel_temporal_filter_bgr_device(mf._ctx, 0, 0, 64, op, 3 * w, None) == state
    assert L.bbme_subpel_temporal_filter_bgr_chain_device(mf._ctx, 0, 1, 64, op, 3 * w, 0, None) == _capi.ERR_UNSUPPORTED
    mf.estimate_async()
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # a forward estimate is none either
    mf.estimate_bidirectional_async()
    first, stats = mf.temporal_filter_subpel_bgr(64), mf.temporal_filter_subpel_bgr_stats(64)
    assert L.bbme_subpel_temporal_filter_bgr_device(mf._ctx, 0, 0, 64, op, 3 * w, None) == 0
    mf.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)
    assert L.bbme_subpel_temporal_filter_bgr_chain_device(mf._ctx, 0, 1, 64, op, 3 * w, 0, None) == _capi.ERR_UNSUPPORTED   # off a chain
    grey = mf.temporal_filter_subpel(64)
    mf.set_frames(g1, g2)                                  # a grey setter withdraws the colour
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter_subpel(64), grey)                     # the same luma: the grey filter stands
    assert [_status(bbme, c) for c in calls] == [state] * 3
    mf.set_frames(c1, c2)
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # colour again, but no fields
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter_subpel_bgr(64), first) and mf.temporal_filter_subpel_bgr_stats(64) == stats
    # the entry point that takes frames and grids needs neither frames nor fields nor stored colour
    mf.set_frames(g1, g2)
    CH, CW = mf.cells_shape
    z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    cur = torch.full((h, w, 3), 9, dtype=torch.uint8, device="cuda")
    mf.cells_temporal_filter_subpel_bgr_device(cur, None, cur, None, z, 64, out=out)
    mf.synchronize()
    assert bool((out == 9).all())
    mf.close()


def test_changes_no_state_and_refuses_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    mf = bbme.MFChain(video[:3], search, block)
    mf.estimate_bidirectional_async()
    h, w = VIDEO[1], VIDEO[0]
    CH, CW = mf.cells_shape

    def state():
        return dict(cells=[mf.get_pair_cells(p) for p in range(2)], back=[mf.get_pair_backward_cells(p) for p in range(2)],
                    planes=[mf.get_slot_plane(l, s) for l in range(3) for s in range(3)],
                    colour=[mf.frame_bgr_tensor(p, w_).cpu().numpy() for p, w_ in ((0, 0), (0, 1), (1, 1))],
                    flow=mf.get_pair_flow(1), grey=mf.temporal_filter_run_subpel(64), integer=mf.temporal_filter_run_bgr(64),
                    half=mf.interpolate_subpel_bgr(1, 2, pair=1))

    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            for x, y in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]):
                assert np.array_equal(x, y), k

    before = state()
    frames = [mf.frame_bgr_tensor(p, w_).clone() for p, w_ in ((0, 0), (0, 1), (1, 1))]
    qp = torch.from_numpy(mf.get_pair_subpel_cells(0, "backward")).cuda()
    qn = torch.from_numpy(mf.get_pair_subpel_cells(1, "forward")).cuda()
    out = torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda")
    wmap = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    run = mf.temporal_filter_run_subpel_bgr(64)
    stats = mf.temporal_filter_subpel_bgr_stats(64, "all")
    mf.cells_temporal_filter_subpel_bgr_device(frames[1], frames[0], frames[2], qp, qn, 64, out=out[0], weights=wmap, stats=st)
    mf.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), run[1]) and tuple(st.cpu().tolist()) == _stats(stats[1])
    # the other getters' scratch and quarter-pel buffers and the filter's are independent
    mf.temporal_filter_subpel_stats(64, "all")
    mf.temporal_filter_bgr_stats(64, "all")
    mf.get_frame_filtered_subpel(0, 1, 64)
    mf.get_pair_motion_compensated_subpel(0)
    assert np.array_equal(mf.temporal_filter_run_subpel_bgr(64), run) and mf.temporal_filter_subpel_bgr_stats(64, "all") == stats
    same(before, state())
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    buf = np.zeros((h, w, 3), np.uint8)
    s12 = (C.c_ulonglong * 12)()
    c_, p_, n_, qp_, qn_, o_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (frames[1], frames[0], frames[2], qp, qn, out, wmap, st))

    def cells(p=p_, c=c_, n=n_, bp=3 * w, a=qp_, b=qn_, qpitch=CW, thr=64, win=None, o=o_, op=3 * w, m=m_, mp=CW, s=s_):
        return L.bbme_cells_subpel_temporal_filter_bgr_device(ctx, p, c, n, bp, a, b, qpitch, thr, win, o, op, m, mp, s, None)

    def own(pair=0, which=0, thr=64, o=o_, op=3 * w):
        return L.bbme_subpel_temporal_filter_bgr_device(ctx, pair, which, thr, o, op, None)

    def run_of(first=0, count=3, thr=64, o=o_, op=3 * w, os=3 * h * w):
        return L.bbme_subpel_temporal_filter_bgr_chain_device(ctx, first, count, thr, o, op, os, None)

    def host(pair=0, which=0, thr=64, o=buf.ctypes.data):
        return L.bbme_get_subpel_temporal_filtered_bgr_host(ctx, pair, which, thr, o)

    assert cells() == 0 and own() == 0 and run_of() == 0 and host() == 0
    assert cells(p=None, a=None) == 0 and cells(n=None, b=None) == 0
    assert cells(p=None, a=None, n=None, b=None) == inv                          # no neighbour at all
    assert cells(p=None) == inv and cells(a=None) == inv and cells(n=None) == inv and cells(b=None) == inv
    assert cells(c=None) == inv
    assert cells(o=None, m=None, s=None) == inv                                  # nothing asked for
    assert cells(qpitch=CW - 1) == inv and cells(qpitch=0) == inv                # the grids' pitch
    for frame in (c_, p_, n_):                                                   # an output inside an input frame
        assert cells(o=frame) == inv
    assert cells(o=C.c_void_p(c_.value + 3 * w)) == inv and cells(n=None, b=None, o=n_) == 0
    assert cells(o=None) == 0 and cells(m=None) == 0 and cells(s=None) == 0 and cells(o=None, m=None) == 0
    assert own(o=None) == inv and run_of(o=None) == inv and host(o=None) == inv
    assert L.bbme_subpel_temporal_filter_bgr_stats(ctx, 64, None, None) == inv
    for thr in (0, -5, 1022):
        assert cells(thr=thr) == inv and own(thr=thr) == inv and run_of(thr=thr) == inv and host(thr=thr) == inv, thr
        assert L.bbme_subpel_temporal_filter_bgr_stats(ctx, thr, None, s12) == inv
    for pair in (-1, 2):
        assert own(pair=pair) == inv and host(pair=pair) == inv
    for which in (-1, 2):
        assert own(which=which) == inv and host(which=which) == inv
    for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (1, -1)):
        assert run_of(first=first, count=count) == inv, (first, count)
    assert run_of(first=2, count=1) == 0 and run_of(first=1, count=2) == 0
    assert cells(op=3 * w - 1) == inv and own(op=3 * w - 1) == inv and run_of(op=3 * w - 1) == inv      # out_pitch < 3 W
    assert cells(bp=3 * w - 1) == inv                                            # bgr_pitch < 3 W
    assert cells(mp=CW - 1) == inv
    assert cells(mp=CW - 1, m=None) == 0 and cells(op=3 * w - 1, o=None) == 0    # a pitch of nothing is not looked at
    assert run_of(count=2, os=3 * h * w - 1) == inv
    assert run_of(count=1, os=0) == 0                                            # one frame has no stride
    for win in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (CW - 7, 0, 8, 8), (0, CH - 7, 8, 8), (0, 0, CW + 1, CH)):
        w4 = (C.c_int * 4)(*win)
        assert cells(win=w4) == inv, win
        assert L.bbme_subpel_temporal_filter_bgr_stats(ctx, 64, w4, s12) == inv, win
    assert L.bbme_subpel_temporal_filter_bgr_stats(ctx, 64, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s12) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_subpel_bgr_device(frames[1], frames[0], None, qp[:, :CW - 2], None, 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_subpel_bgr_device(frames[1], frames[0][:, :w - 1], None, qp, None, 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.temporal_filter_run_subpel_bgr(64, 2, 3)
    assert e.value.status == inv
    mf.synchronize()
    same(before, state())
    assert np.array_equal(mf.temporal_filter_run_subpel_bgr(64), run)
    # the captured graphs replay to the same field
    mf.estimate_bidirectional_async()
    same(before, state())
    mf.close()


DENOISE_STRENGTH = 96


@pytest.fixture(scope="module")
def denoise_reference(bbme):
    """Seven 200 x 136 colour frames and, per frame, the rule in numpy on (previous, current, next) with the integer fields of
    single contexts refined on the CPU on the padded luma planes"""
    video = _colour7(bbme)
    ref = _video_reference(bbme, "denoise", video)
    return video, [_video_rule(video, ref, f, DENOISE_STRENGTH)[0] for f in range(7)]


@pytest.mark.parametrize("in_flight,batch", [(2, 1), (4, 2)])
def test_denoise_frames_subpel_bgr(bbme, denoise_reference, in_flight, batch):
    """in_flight=4, batch=2: two contexts, a carried round each and the segment boundary at frame 3; in_flight=2, batch=1: every
    frame but the ends is a boundary frame, filtered from the copies of colour frames and quarter-pel grids."""
    from blockbasedmotionestimation_amd.sequence import denoise_frames
    search, block = VIDEO_PARAMS
    video, exp = denoise_reference
    keep = [v.copy() for v in video]
    got = denoise_frames(video, search, block, DENOISE_STRENGTH, in_flight=in_flight, batch=batch, subpel_bgr=True)
    assert len(got) == 7
    for v, k in zip(video, keep):
        assert np.array_equal(v, k)
    for f in range(7):
        assert got[f].shape == (VIDEO[1], VIDEO[0], 3) and got[f].dtype == np.uint8
        assert np.array_equal(got[f], exp[f]), f
    assert any(not np.array_equal(got[f], video[f]) for f in range(7))


def test_denoise_frames_refuses_grey_frames_with_subpel_bgr(bbme):
    from blockbasedmotionestimation_amd.sequence import denoise_frames
    search, block = VIDEO_PARAMS
    grey = bbme.synth_video(VIDEO[0], VIDEO[1], 3, VIDEO[3], max_motion=VIDEO[4])
    with pytest.raises(ValueError):
        denoise_frames(grey, search, block, 96, subpel_bgr=True)


def test_cli_writes_the_quarter_pel_denoised_colour_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    video = colour_video(bbme)
    c1, c2 = (np.ascontiguousarray(v[:72, :96]) for v in video[:2])
    _write_ppm(tmp_path / "f1.ppm", c1)
    _write_ppm(tmp_path / "f2.ppm", c2)
    args = ["--levels", "3", "--block", "16", "--search", "30", "--no-upsample", "--strength", "96"]
    r = subprocess.run([_build.CLI, str(tmp_path / "f1.ppm"), str(tmp_path / "f2.ppm")] + args + ["--denoise-subpel", str(tmp_path / "dq")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(c1, c2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    px, py = mf.padding_x, mf.padding_y
    for which in (0, 1):
        frame = mf.temporal_filter_subpel_bgr(96, which)
        assert (tmp_path / ("dq_%d.ppm" % (which + 1))).read_bytes() == \
            b"P6\n96 72\n255\n" + np.ascontiguousarray(frame[..., ::-1]).tobytes(), which
        luma = mf.temporal_filter_subpel(96, which)[py:py + 72, px:px + 96]
        assert (tmp_path / ("dq_%d.pgm" % (which + 1))).read_bytes() == b"P5\n96 72\n255\n" + luma.tobytes(), which
    mf.close()
    # grey frames: the luma files alone, unchanged
    for name, c in (("g1.pgm", c1), ("g2.pgm", c2)):
        (tmp_path / name).write_bytes(b"P5\n96 72\n255\n" + np_bgr_to_gray(c).tobytes())
    r = subprocess.run([_build.CLI, str(tmp_path / "g1.pgm"), str(tmp_path / "g2.pgm")] + args + ["--denoise-subpel", str(tmp_path / "gr")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "gr_1.pgm").exists() and (tmp_path / "gr_2.pgm").exists()
    assert not (tmp_path / "gr_1.ppm").exists() and not (tmp_path / "gr_2.ppm").exists()
    assert (tmp_path / "gr_1.pgm").read_bytes() == (tmp_path / "dq_1.pgm").read_bytes()          # the luma of the colour run
