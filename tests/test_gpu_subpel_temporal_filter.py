"""Temporal filtering along quarter-pel grids on the GPU (include/bbme.h, "SUBPEL TEMPORAL FILTER RULE"): k_subpel_temporal_filter
gives exactly the numpy restatement of tests/test_subpel_temporal_filter_cpu.py on the context's own planes and refined fields and on
injected planes and grids -- every fraction, cell rows that are and are not whole runs, caller pitches that are not multiples of 4,
strided grids, windows that cut runs, each output alone, vectors on and past every edge and int16 extremes under guard bands --; with
4 x integer grids it gives k_temporal_filter's bytes on the division tables; both divisions are exact on sampled costs; chains filter
every slot from both sides, batches from one; the calls change no context state and refuse bad arguments; sequence.denoise_frames
filters every frame of a video along quarter-pel fields across rounds and contexts; bbme_cli --denoise-subpel writes the frames."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _cuda, _embed, _odd_window, _stats_of, _write_pgm
from test_gpu_bidirectional import CASES, _frames
from test_interpolation_cpu import extreme_grids, oracle_grids, random_grids
from test_subpel_interpolation_cpu import fraction_grids
from test_subpel_temporal_filter_cpu import (edge_grid, near_frames, np_subpel_temporal_filter, sampled_cost_check, sampled_cost_table)
from test_temporal_filter_cpu import (S23_THR, STAT_KEYS, np_temporal_filter, s23_table_planes, s_table_check, s_table_planes,
                                      thr_table_expected, thr_table_planes)

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

VIDEO = (200, 136, 4, 77, 6)                               # synth_video(width, height, frames, seed, max_motion=...)
VIDEO_PARAMS = ([30, 30, 30], [16, 16, 16])


def _device_filter(mf, Cur, P, QP, N, QN, thr, window=None, pitch_extra=0, map_extra=0, q_extra=0, stream=None,
                   want=("out", "map", "stats"), integer=False):
    """cells_temporal_filter_subpel_device (integer: cells_temporal_filter_device) on host planes and grids -> (frame (H0, W0), map
    (CH, CW), stats tuple) as numpy / tuple, None where not asked for; rows of the frame are pitch_extra bytes, of the map map_extra
    bytes and of both grids q_extra cells further apart than packed; the bytes and cells in between stay untouched."""
    import torch
    CH, CW = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    tc, tp, tn = (_cuda(a) for a in (Cur, P, N))
    grids = []
    for Q in (QP, QN):
        if Q is None:
            grids.append(None)
            continue
        t = torch.full((CH, CW + q_extra, 2), 0x7777, dtype=torch.int16, device="cuda")
        t[:, :CW] = _cuda(np.asarray(Q, np.int16))
        grids.append(t)
    out = torch.full((H0, W0 + pitch_extra), 0xAA, dtype=torch.uint8, device="cuda") if "out" in want else None
    wmap = torch.full((CH, CW + map_extra), 0xAA, dtype=torch.uint8, device="cuda") if "map" in want else None
    st = torch.zeros(4, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    views = [None if t is None else (t[:, :CW] if q_extra else t[:, :CW].contiguous()) for t in grids]
    kw = dict(out=None if out is None else out[:, :W0], weights=None if wmap is None else wmap[:, :CW], stats=st, window=window)
    if integer:
        mf.cells_temporal_filter_device(tc, tp, tn, views[0], views[1], thr, **kw)
    else:
        mf.cells_temporal_filter_subpel_device(tc, tp, tn, views[0], views[1], thr, stream=None if stream is None else stream.cuda_stream,
                                               **kw)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    assert out is None or not pitch_extra or bool((out[:, W0:] == 0xAA).all())
    assert wmap is None or not map_extra or bool((wmap[:, CW:] == 0xAA).all())
    for t in grids:
        assert t is None or bool((t[:, CW:] == 0x7777).all())
    return (None if out is None else out[:, :W0].cpu().numpy(), None if wmap is None else wmap[:, :CW].cpu().numpy(),
            None if st is None else tuple(st.cpu().tolist()))


def _assert_device_equals_numpy(mf, Cur, P, QP, N, QN, thr, window=None, what=None, **kw):
    out, wmap, st = _device_filter(mf, Cur, P, QP, N, QN, thr, window, **kw)
    exp = np_subpel_temporal_filter(Cur, P, QP, N, QN, thr, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert out is None or np.array_equal(out, exp[0]), tag
    assert wmap is None or np.array_equal(wmap, exp[1]), tag
    assert st is None or st == exp[2], tag
    return exp


def _refined(bbme, I1, I2, fwd, bwd):
    """The two fields refined on the CPU: the grid on image 1 into image 2 and the grid on image 2 into image 1"""
    return bbme.subpel_cells(I1, I2, fwd)[0], bbme.subpel_cells(I2, I1, bwd)[0]


@pytest.mark.parametrize("name", ["cfg1_like", "border_motion"])
def test_equals_numpy_on_the_oracles_refined_fields(bbme, oracle, name):
    import torch
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    fwd, bwd = oracle_grids(bbme, oracle, name)
    mf = bbme.MF(f1, f2, search, block, upsample=up)
    mf.estimate_bidirectional_async()
    I1, I2 = mf.get_level_planes(0)
    qf, qb = _refined(bbme, I1, I2, fwd, bwd)
    assert np.array_equal(mf.subpel_cells("forward"), qf) and np.array_equal(mf.subpel_cells("backward"), qb)
    assert (qf & 3).any() and (qb & 3).any()
    odd = _odd_window(mf)
    own = [(I1, None, None, I2, qf), (I2, I1, qb, None, None)]
    for thr in (1, 64, 1021):
        for which in (0, 1):
            assert np.array_equal(mf.temporal_filter_subpel(thr, which), np_subpel_temporal_filter(*own[which], thr)[0]), (thr, which)
        for win, np_win in ((None, mf.default_cell_window()), ("all", None), (odd, odd)):
            got = mf.temporal_filter_subpel_stats(thr, win)
            assert [_stats(g) for g in got] == [np_subpel_temporal_filter(*own[which], thr, np_win)[2] for which in (0, 1)], (thr, win)
    # the same through the entry point that takes any planes and grids
    _assert_device_equals_numpy(mf, *own[0], 64, what="image 1, refined grid")
    _assert_device_equals_numpy(mf, *own[1], 64, odd, "image 2, refined grid", q_extra=3)
    _assert_device_equals_numpy(mf, I2, I1, qb, I1, qb, 64, odd, "image 2 between two copies of image 1", pitch_extra=3, map_extra=1)
    _assert_device_equals_numpy(mf, I2, I1, qb, I1, qb, 1, what="side stream", stream=torch.cuda.Stream())
    # the injected planes and grids left the context's own alone
    assert np.array_equal(mf.temporal_filter_subpel(64), np_subpel_temporal_filter(*own[0], 64)[0])
    mf.close()


# 200 x 136 at [30] * 3 / [16] * 3 pads to 256 x 192 (W0 = 0 mod 8: whole runs); 132 x 100 at [12] / [2] is not padded (W0 = 4 mod 8:
# 66 cells, the last run of a cell row holds 2 cells, and rows of 132 bytes put every second pixel row off 8-byte alignment)
INJECTED = [(200, 136, [30] * 3, [16] * 3), (132, 100, [12], [2])]


@pytest.mark.parametrize("w,h,search,block", INJECTED)
def test_every_fraction_pitches_windows_and_outputs(bbme, w, h, search, block):
    z = np.zeros((h, w), np.uint8)
    mf = bbme.MF(z, z, search, block)
    H0, W0 = mf.padded_height, mf.padded_width
    CH, CW = mf.cells_shape
    assert (W0 % 8, CW % 4) == ((0, 0) if w == 200 else (4, 2))
    Cur, P, N = near_frames(H0, W0, w)
    qp, qn = fraction_grids(H0, W0, h)
    exp = _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 255, None, "fractions")
    every = {(a, b) for a in range(4) for b in range(4)}
    for wbits, Q in ((exp[1] & 0x0f, qp), (exp[1] >> 4, qn)):                     # every fraction class was taken, by both neighbours
        assert {(int(a) & 3, int(b) & 3) for a, b in Q[wbits > 0]} == every
    cut = (CW - 7, 2, 7, CH - 5)                           # reaches the last run of the rows
    inner = (3, 1, 5, 3)                                   # starts and ends inside runs
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 64, cut, "pitch + 1", pitch_extra=1, map_extra=1)
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 1021, inner, "pitch + 3, strided grids", pitch_extra=3, map_extra=1, q_extra=3)
    _assert_device_equals_numpy(mf, Cur, P, qp, None, None, 1021, cut, "previous only", q_extra=3)
    _assert_device_equals_numpy(mf, Cur, None, None, N, qn, 64, None, "next only", pitch_extra=1)
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 255, what="frame only", want=("out",), pitch_extra=3)
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 1021, what="map only", want=("map",), map_extra=1)
    _assert_device_equals_numpy(mf, Cur, P, qp, N, qn, 64, cut, "statistics only", want=("stats",), q_extra=3)
    # property 1 on random integer grids: 4 x the grid through K13 is K9 on the grid
    rng = np.random.default_rng(h)
    gp, gn = random_grids(CH, CW, rng, reach=2)
    for thr, win in ((64, cut), (1021, None)):
        old = _device_filter(mf, Cur, P, gp, N, gn, thr, win, integer=True)
        new = _device_filter(mf, Cur, P, 4 * gp, N, 4 * gn, thr, win)
        assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]) and old[2] == new[2], thr
        assert old[2] == np_temporal_filter(Cur, P, gp, N, gn, thr, win)[2]
    mf.close()


def _guarded_results(bbme):
    """Edge validity and int16 extremes through cells_temporal_filter_subpel_device, and the own-context calls of a single and a
    chain context -> (contexts, sha256 of every result)"""
    w, h = 132, 100
    z = np.zeros((h, w), np.uint8)
    mf = bbme.MF(z, z, [12], [2])
    H0, W0 = mf.padded_height, mf.padded_width
    assert (W0, H0) == (w, h)
    rng = np.random.default_rng(5)
    Cur, P, N = (rng.integers(100, 104, (H0, W0)).astype(np.uint8) for _ in range(3))
    Q, cells = edge_grid(H0, W0)
    results = []
    for p, a, q, b in ((P, Q, N, Q), (P, Q, None, None), (None, None, N, Q)):
        out, wmap, st = _assert_device_equals_numpy(mf, Cur, p, a, q, b, 1021, None, "edges", pitch_extra=1)
        for cx, cy, valid in cells:
            wp, wn = wmap[cy, cx] & 0x0f, wmap[cy, cx] >> 4
            assert (wp > 0) == (valid and p is not None) and (wn > 0) == (valid and q is not None), (cx, cy, valid)
            if not valid:
                assert np.array_equal(out[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2], Cur[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2])
        results += [out, wmap, np.array(st)]
    xp, xn = extreme_grids(H0 // 2, W0 // 2, rng)
    for thr in (1, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, Cur, P, xp, N, xn, thr, None, "int16 extremes", q_extra=3)
        assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)
    mf.close()
    frames = bbme.synth_video(136, 104, 3, 5, max_motion=4)
    single = bbme.MF(frames[0], frames[1], [20, 20], [8, 8])
    chain = bbme.MFChain(frames, [20, 20], [8, 8])
    for ctx in (single, chain):
        ctx.estimate_bidirectional_async()
    results += [single.temporal_filter_subpel(64, 0), single.temporal_filter_subpel(64, 1), chain.temporal_filter_run_subpel(96)]
    results += [np.array([_stats(s) for s in ctx.temporal_filter_subpel_stats(64, "all")]) for ctx in (single, chain)]
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
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_subpel_temporal_filter as t; t._guard_child()" % (
        tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:5] == [digest, "buffer=1", "violations=0", "after_close=0"], line[0]


@pytest.fixture(scope="module")
def table_context(bbme):
    """A one-level 132 x 100 context: the division tables are injected as tensors, its own frames do not matter."""
    z = np.zeros((100, 132), np.uint8)
    mf = bbme.MF(z, z, [12], [2])
    assert (mf.padded_width, mf.padded_height) == (132, 100)
    yield mf
    mf.close()


def _assert_property_1(mf, Cur, P, GP, N, GN, thr):
    """K13 on 4 x the grids gives K9's frame, map and statistics on the grids"""
    old = _device_filter(mf, Cur, P, GP, N, GN, thr, integer=True)
    q = [None if g is None else (4 * g.astype(np.int32)).astype(np.int16) for g in (GP, GN)]
    new = _device_filter(mf, Cur, P, q[0], N, q[1], thr)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]) and old[2] == new[2], thr
    return new


def test_property_1_on_the_division_tables(table_context):
    mf = table_context
    H0, W0 = mf.padded_height, mf.padded_width
    CH, CW = mf.cells_shape
    z = np.zeros((CH, CW, 2), np.int16)
    Cur, N, cost = thr_table_planes()                      # 92 x 92 inside the 132 x 100 plane; the rest is 0 against 0: weight 8
    Cur, N = _embed(Cur, H0, W0), _embed(N, H0, W0)
    for thr in (1, 2, 3, 7, 64, 255, 1020, 1021):
        exp = np.full((CH, CW), 8, np.int64)
        exp[:cost.shape[0], :cost.shape[1]] = thr_table_expected(cost, thr)
        _, wmap, _ = _assert_property_1(mf, Cur, None, None, N, z, thr)
        assert np.array_equal(wmap >> 4, exp) and not (wmap & 0x0f).any()
    Cur, P, N, expect_w = s_table_planes()                 # 132 x 100, the context's own size
    out, wmap, _ = _assert_property_1(mf, Cur, P, z, N, z, 64)
    s_table_check(Cur, P, N, expect_w, out, wmap)
    Cur, P, N, expect_w = s23_table_planes()
    out, wmap, _ = _assert_property_1(mf, Cur, P, z, N, z, S23_THR)
    s_table_check(Cur, P, N, expect_w, out, wmap, pairs=[(8, 7)], ends=False)


def test_division_on_sampled_costs_in_the_kernel(bbme):
    Cur, X, grid, k = sampled_cost_table()
    mf = bbme.MF(Cur, Cur, [12], [2])
    assert (mf.padded_height, mf.padded_width) == Cur.shape
    for thr in (1, 64, 1021):
        out, wmap, _ = _assert_device_equals_numpy(mf, Cur, None, None, X, grid, thr)
        sampled_cost_check(k, thr, out, wmap >> 4)
        out, wmap, _ = _assert_device_equals_numpy(mf, Cur, X, grid, None, None, thr)
        sampled_cost_check(k, thr, out, wmap & 0x0f)
    mf.close()


def test_chain_filters_every_slot_and_batch_one_side(bbme):
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    chain = bbme.MFChain(video, search, block)
    chain.estimate_bidirectional_async()
    planes = [chain.get_slot_plane(0, s) for s in range(4)]
    qf = [chain.get_pair_subpel_cells(p, "forward") for p in range(3)]
    qb = [chain.get_pair_subpel_cells(p, "backward") for p in range(3)]
    for p in range(3):                                     # the refinement on the CPU of the chain's integer cells
        f, b = _refined(bbme, planes[p], planes[p + 1], chain.get_pair_cells(p), chain.get_pair_backward_cells(p))
        assert np.array_equal(qf[p], f) and np.array_equal(qb[p], b), p
    win = _odd_window(chain)

    def rule(f, thr, window=None):
        return np_subpel_temporal_filter(planes[f], planes[f - 1] if f > 0 else None, qb[f - 1] if f > 0 else None,
                                         planes[f + 1] if f < 3 else None, qf[f] if f < 3 else None, thr, window)

    for thr in (64, 1021):
        exp = [rule(f, thr)[0] for f in range(4)]
        run = chain.temporal_filter_run_subpel(thr)
        assert run.shape == (4,) + planes[0].shape
        for f in range(4):
            assert np.array_equal(run[f], exp[f]), (thr, f)
        assert np.array_equal(chain.temporal_filter_run_subpel(thr, 1, 2), np.stack(exp[1:3]))
        assert np.array_equal(chain.temporal_filter_run_subpel(thr, 3, 1)[0], exp[3])
        assert np.array_equal(chain.temporal_filter_run_subpel(thr, 0, 1)[0], exp[0])
        for p in range(3):
            assert np.array_equal(chain.get_frame_filtered_subpel(p, 0, thr), exp[p]), (thr, p)
            assert np.array_equal(chain.get_frame_filtered_subpel(p, 1, thr), exp[p + 1]), (thr, p)   # (p, 1) and (p + 1, 0): one frame
        assert np.array_equal(chain.temporal_filter_subpel(thr), exp[0])
        for w, np_win in ((None, chain.default_cell_window()), ("all", None), (win, win)):
            assert [_stats(s) for s in chain.temporal_filter_subpel_stats(thr, w)] == [rule(f, thr, np_win)[2] for f in range(4)], (thr, w)
    inner = rule(1, 64)
    assert (inner[1] & 0x0f).any() and (inner[1] >> 4).any()                       # inner frames take from both sides
    chain.close()
    # a batch of the same pairs: image 1 forward-only, image 2 backward-only
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(3)], search, block)
    batch.estimate_bidirectional_async()
    exp_stats = []
    for p in (2, 0, 1):
        one = np_subpel_temporal_filter(planes[p], None, None, planes[p + 1], qf[p], 64)
        two = np_subpel_temporal_filter(planes[p + 1], planes[p], qb[p], None, None, 64)
        assert np.array_equal(batch.get_frame_filtered_subpel(p, 0, 64), one[0]), p
        assert np.array_equal(batch.get_frame_filtered_subpel(p, 1, 64), two[0]), p
    for p in range(3):
        exp_stats += [np_subpel_temporal_filter(planes[p], None, None, planes[p + 1], qf[p], 64, win)[2],
                      np_subpel_temporal_filter(planes[p + 1], planes[p], qb[p], None, None, 64, win)[2]]
    assert [_stats(s) for s in batch.temporal_filter_subpel_stats(64, win)] == exp_stats
    batch.close()


def test_needs_a_valid_pair_of_fields(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    mf = bbme.MF(video[0], video[1], search, block)

    def state_errors(ctx, what):
        calls = [lambda: ctx.temporal_filter_subpel(64), lambda: ctx.temporal_filter_subpel(64, 1),
                 lambda: ctx.temporal_filter_subpel_stats(64)]
        if isinstance(ctx, bbme.MFChain):
            calls.append(lambda: ctx.temporal_filter_run_subpel(64))
        for call in calls:
            with pytest.raises(bbme.BbmeError) as e:
                call()
            assert e.value.status == _capi.ERR_STATE, what

    state_errors(mf, "before any estimate")
    out = torch.zeros((mf.padded_height, mf.padded_width), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    op = C.c_void_p(out.data_ptr())
    assert L.bbme_subpel_temporal_filter_device(mf._ctx, 0, 0, 64, op, mf.padded_width, None) == _capi.ERR_STATE
    assert L.bbme_subpel_temporal_filter_chain_device(mf._ctx, 0, 1, 64, op, mf.padded_width, 0, None) == _capi.ERR_UNSUPPORTED
    mf.estimate_async()
    state_errors(mf, "after bbme_estimate")
    mf.estimate_bidirectional_async()
    first = mf.temporal_filter_subpel(64)
    assert L.bbme_subpel_temporal_filter_device(mf._ctx, 0, 0, 64, op, mf.padded_width, None) == 0
    mf.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)
    assert L.bbme_subpel_temporal_filter_chain_device(mf._ctx, 0, 1, 64, op, mf.padded_width, 0, None) == _capi.ERR_UNSUPPORTED
    mf.set_frames(video[0], video[1])
    state_errors(mf, "after a frame setter")
    # the entry point that takes planes and grids needs neither frames nor fields
    z = torch.zeros((out.shape[0] // 2, out.shape[1] // 2, 2), dtype=torch.int16, device="cuda")
    cur = torch.full_like(out, 9)
    mf.cells_temporal_filter_subpel_device(cur, None, cur, None, z, 64, out=out)
    mf.synchronize()
    assert bool((out == 9).all())
    mf.close()
    chain = bbme.MFChain(video[:3], search, block)
    chain.estimate_bidirectional_async()
    chain.temporal_filter_run_subpel(64)
    chain.advance([video[3]])
    state_errors(chain, "between advance and the estimate")
    chain.close()


def test_changes_no_state_and_refuses_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    mf = bbme.MFChain(video[:3], search, block)
    mf.estimate_bidirectional_async()

    def state():
        return dict(flow=mf.get_pair_flow(1), cells=mf.get_pair_cells(0), back=mf.get_pair_backward_cells(1),
                    filtered=mf.temporal_filter_run(64), stats=mf.temporal_filter_stats(64, "all"), half=mf.get_pair_interpolated(1),
                    sub=mf.get_pair_interpolated_subpel(0), mcq=mf.get_pair_motion_compensated_subpel(1))

    def digest(s):
        return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() if isinstance(v, np.ndarray) else v for k, v in s.items()}

    before = digest(state())
    CH, CW = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    planes = [mf.frame_plane_tensor(p, w).clone() for p, w in ((0, 0), (0, 1), (1, 1))]
    qp = torch.from_numpy(mf.get_pair_subpel_cells(0, "backward")).cuda()
    qn = torch.from_numpy(mf.get_pair_subpel_cells(1, "forward")).cuda()
    out = torch.zeros((3, H0, W0), dtype=torch.uint8, device="cuda")
    wmap = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    run = mf.temporal_filter_run_subpel(64)
    stats = mf.temporal_filter_subpel_stats(64, "all")
    mf.cells_temporal_filter_subpel_device(planes[1], planes[0], planes[2], qp, qn, 64, out=out[0], weights=wmap, stats=st)
    mf.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), run[1]) and tuple(st.cpu().tolist()) == _stats(stats[1])
    # the other subpel getters' quarter-pel buffers and the filter's are independent
    mf.get_pair_motion_compensated_subpel(0)
    mf.get_pair_interpolated_subpel(1)
    mf.temporal_filter_stats(64, "all")
    assert np.array_equal(mf.temporal_filter_run_subpel(64), run) and mf.temporal_filter_subpel_stats(64, "all") == stats
    assert digest(state()) == before
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    buf = np.zeros((H0, W0), np.uint8)
    s12 = (C.c_ulonglong * 12)()
    c_, p_, n_, qp_, qn_, o_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (planes[1], planes[0], planes[2], qp, qn, out, wmap, st))

    def cells(p=p_, c=c_, n=n_, a=qp_, b=qn_, qpitch=CW, thr=64, win=None, o=o_, op=W0, m=m_, mp=CW, s=s_):
        return L.bbme_cells_subpel_temporal_filter_device(ctx, p, c, n, a, b, qpitch, thr, win, o, op, m, mp, s, None)

    def own(pair=0, which=0, thr=64, o=o_, op=W0):
        return L.bbme_subpel_temporal_filter_device(ctx, pair, which, thr, o, op, None)

    def run_of(first=0, count=3, thr=64, o=o_, op=W0, os=H0 * W0):
        return L.bbme_subpel_temporal_filter_chain_device(ctx, first, count, thr, o, op, os, None)

    def host(pair=0, which=0, thr=64, o=buf.ctypes.data):
        return L.bbme_get_subpel_temporal_filtered_host(ctx, pair, which, thr, o)

    assert cells() == 0 and own() == 0 and run_of() == 0 and host() == 0
    assert cells(p=None, a=None) == 0 and cells(n=None, b=None) == 0
    assert cells(p=None, a=None, n=None, b=None) == inv                          # no neighbour at all
    assert cells(p=None) == inv and cells(a=None) == inv and cells(n=None) == inv and cells(b=None) == inv
    assert cells(c=None) == inv
    assert cells(o=None, m=None, s=None) == inv                                  # nothing asked for
    assert cells(qpitch=CW - 1) == inv and cells(qpitch=0) == inv                # the grids' pitch
    for plane in (c_, p_, n_):                                                   # an output inside an input plane
        assert cells(o=plane) == inv
    assert cells(o=None) == 0 and cells(m=None) == 0 and cells(s=None) == 0 and cells(o=None, m=None) == 0
    assert own(o=None) == inv and run_of(o=None) == inv and host(o=None) == inv
    assert L.bbme_subpel_temporal_filter_stats(ctx, 64, None, None) == inv
    for thr in (0, -5, 1022):
        assert cells(thr=thr) == inv and own(thr=thr) == inv and run_of(thr=thr) == inv and host(thr=thr) == inv, thr
        assert L.bbme_subpel_temporal_filter_stats(ctx, thr, None, s12) == inv
    for pair in (-1, 2):
        assert own(pair=pair) == inv and host(pair=pair) == inv
    for which in (-1, 2):
        assert own(which=which) == inv and host(which=which) == inv
    for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (1, -1)):
        assert run_of(first=first, count=count) == inv, (first, count)
    assert run_of(first=2, count=1) == 0 and run_of(first=1, count=2) == 0
    assert cells(op=W0 - 1) == inv and own(op=W0 - 1) == inv and run_of(op=W0 - 1) == inv
    assert cells(mp=CW - 1) == inv
    assert run_of(count=2, os=H0 * W0 - 1) == inv
    for win in ((-1, 0, 8, 8), (0, 0, 0, 8), (CW - 7, 0, 8, 8), (0, CH - 7, 8, 8), (0, 0, CW + 1, CH)):
        w4 = (C.c_int * 4)(*win)
        assert cells(win=w4) == inv, win
        assert L.bbme_subpel_temporal_filter_stats(ctx, 64, w4, s12) == inv, win
    assert L.bbme_subpel_temporal_filter_stats(ctx, 64, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s12) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_subpel_device(planes[1], planes[0], None, qp[:, :CW - 2], None, 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.temporal_filter_run_subpel(64, 2, 3)
    assert e.value.status == inv
    mf.synchronize()
    assert digest(state()) == before
    assert np.array_equal(mf.temporal_filter_run_subpel(64), run)
    mf.close()


def test_upsampled_context_filters_its_x4_planes(bbme):
    w, h, search, block, _, _, up = CASES["x4"]
    f1, f2 = _frames(bbme, "x4")
    mf = bbme.MF(f1, f2, search, block, upsample=up)
    mf.estimate_bidirectional_async()
    I1, I2 = mf.get_level_planes(0)
    assert I1.shape == (mf.padded_height, mf.padded_width) and mf.padded_width >= 4 * w
    qf, qb = _refined(bbme, I1, I2, mf.get_cells(), mf.get_backward_cells())
    exp = [np_subpel_temporal_filter(I1, None, None, I2, qf, 96, mf.default_cell_window()),
           np_subpel_temporal_filter(I2, I1, qb, None, None, 96, mf.default_cell_window())]
    for which in (0, 1):
        assert np.array_equal(mf.temporal_filter_subpel(96, which), exp[which][0]), which
    assert [_stats(s) for s in mf.temporal_filter_subpel_stats(96)] == [e[2] for e in exp]
    mf.close()


DENOISE_VIDEO = (96, 64, 7, 31, 4)
DENOISE_PARAMS = ([30, 30], [16, 16])                      # two levels: a third would be less than two blocks high


@pytest.fixture(scope="module")
def denoise_reference(bbme):
    """7 frames of a 96 x 64 video and, per frame, both rules on (previous, current, next) on the CPU: the integer fields of single
    MF contexts, refined by bbme.subpel_cells for the quarter-pel rule."""
    search, block = DENOISE_PARAMS
    w, h, n = DENOISE_VIDEO[:3]
    video = bbme.synth_video(w, h, n, DENOISE_VIDEO[3], max_motion=DENOISE_VIDEO[4])
    planes, fwd, bwd = [None] * n, [None] * (n - 1), [None] * (n - 1)
    for p in range(n - 1):
        mf = bbme.MF(video[p], video[p + 1], search, block)
        mf.estimate_bidirectional_async()
        planes[p], planes[p + 1] = mf.get_level_planes(0)
        fwd[p], bwd[p] = mf.get_cells(), mf.get_backward_cells()
        px, py = mf.padding_x, mf.padding_y
        mf.close()
    exp, exp_int = [], []
    for f in range(n):
        P, N = (planes[f - 1] if f > 0 else None), (planes[f + 1] if f < n - 1 else None)
        qp = bbme.subpel_cells(planes[f], P, bwd[f - 1])[0] if f > 0 else None
        qn = bbme.subpel_cells(planes[f], N, fwd[f])[0] if f < n - 1 else None
        full = bbme.temporal_filter_cells_subpel(planes[f], P, N, qp, qn, 96)[0]
        exp.append(full[py:py + h, px:px + w])
        full = bbme.temporal_filter_cells(planes[f], P, N, bwd[f - 1] if f > 0 else None, fwd[f] if f < n - 1 else None, 96)[0]
        exp_int.append(full[py:py + h, px:px + w])
    return video, exp, exp_int


@pytest.mark.parametrize("in_flight,batch", [(2, 1), (4, 2)])
def test_denoise_frames_subpel(bbme, denoise_reference, in_flight, batch):
    """in_flight=4, batch=2: two contexts, a carried round each and the segment boundary at frame 3; in_flight=2, batch=1: every
    frame but the ends is a boundary frame, filtered from the copies of quarter-pel grids."""
    from blockbasedmotionestimation_amd import _capi
    from blockbasedmotionestimation_amd.sequence import denoise_frames
    search, block = DENOISE_PARAMS
    video, exp, exp_int = denoise_reference
    w, h, n = DENOISE_VIDEO[:3]
    keep = [v.copy() for v in video]
    got = denoise_frames(video, search, block, 96, in_flight=in_flight, batch=batch, subpel=True)
    assert len(got) == n
    for v, k in zip(video, keep):
        assert np.array_equal(v, k)
    for f in range(n):
        assert got[f].shape == (h, w) and got[f].dtype == np.uint8
        assert np.array_equal(got[f], exp[f]), f
    assert any(not np.array_equal(exp[f], exp_int[f]) for f in range(n))           # the quarter-pel route is another result
    for kw in (dict(), dict(subpel=False)):                                      # the integer route is what it was
        old = denoise_frames(video, search, block, 96, in_flight=in_flight, batch=batch, **kw)
        for f in range(n):
            assert np.array_equal(old[f], exp_int[f]), (kw, f)
    colour = [np.stack([v, v, v], -1) for v in video[:3]]
    with pytest.raises(bbme.BbmeError) as e:
        denoise_frames(colour, search, block, 96, subpel=True)
    assert e.value.status == _capi.ERR_UNSUPPORTED and "integer" in e.value.message and "colour" in e.value.message


def test_cli_writes_the_quarter_pel_denoised_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    f1, f2, _ = bbme.synth_pair(96, 72, 1001, max_motion=3)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    base = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm"), "--levels", "3", "--block", "16", "--search", "30"]
    r = subprocess.run(base + ["--no-upsample", "--denoise-subpel", str(tmp_path / "dq"), "--strength", "96"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    px, py = mf.padding_x, mf.padding_y
    for which in (0, 1):
        frame = mf.temporal_filter_subpel(96, which)[py:py + 72, px:px + 96]
        assert (tmp_path / ("dq_%d.pgm" % (which + 1))).read_bytes() == b"P5\n96 72\n255\n" + frame.tobytes(), which
    mf.close()
    r = subprocess.run(base + ["--no-upsample", "--denoise-subpel", str(tmp_path / "bad"), "--strength", "0"], capture_output=True,
                       text=True)
    assert r.returncode == 2 and "--denoise-subpel" in r.stderr
    assert not (tmp_path / "bad_1.pgm").exists()
