"""Motion-compensated temporal filtering on the GPU (include/bbme.h, "TEMPORAL FILTER RULE"): k_temporal_filter gives exactly
the numpy restatement of the rule (test_temporal_filter_cpu.np_temporal_filter) on the context's own planes and fields, on injected
planes and grids (the oracle's, random, int16 extremes; both neighbours and each alone), with windows, caller pitches that are not
multiples of 4, side streams and geometries whose cell rows end inside a lane's run; both divisions are exact for every numerator;
chains filter every slot from both sides, batches from one; the calls change no context state and refuse bad arguments;
sequence.denoise_frames filters every frame of a video from its true neighbours across rounds and contexts."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _cuda, _embed, _odd_window, _stats_of, _write_pgm
from test_gpu_bidirectional import CASES, _frames
from test_interpolation_cpu import extreme_grids, oracle_grids, random_grids
from test_temporal_filter_cpu import (S23_THR, STAT_KEYS, THRS, np_temporal_filter, s23_table_planes, s_table_check, s_table_planes,
                                      thr_table_expected, thr_table_planes)

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

VIDEO = (200, 136, 4, 77, 6)                               # synth_video(width, height, frames, seed, max_motion=...)
VIDEO_PARAMS = ([30, 30, 30], [16, 16, 16])


def _device_filter(mf, Cur, P, GP, N, GN, thr, window=None, pitch_extra=0, stream=None, want=("out", "map", "stats")):
    """cells_temporal_filter_device on host planes and grids -> (frame (H0, W0), map (CH, CW), stats tuple) as numpy / tuple, None
    where not asked for; rows of both outputs are pitch_extra bytes further apart than packed."""
    import torch
    CH, CW = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    tc, tp, tn, tgp, tgn = (_cuda(a) for a in (Cur, P, N, GP, GN))
    out = torch.full((H0, W0 + pitch_extra), 0xAA, dtype=torch.uint8, device="cuda") if "out" in want else None
    wmap = torch.full((CH, CW + pitch_extra), 0xAA, dtype=torch.uint8, device="cuda") if "map" in want else None
    st = torch.zeros(4, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    mf.cells_temporal_filter_device(tc, tp, tn, tgp, tgn, thr, out=None if out is None else out[:, :W0],
                                    weights=None if wmap is None else wmap[:, :CW], stats=st, window=window,
                                    hip_stream_handle=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    if pitch_extra:                                        # the bytes between the rows stay untouched
        assert out is None or bool((out[:, W0:] == 0xAA).all())
        assert wmap is None or bool((wmap[:, CW:] == 0xAA).all())
    return (None if out is None else out[:, :W0].cpu().numpy(), None if wmap is None else wmap[:, :CW].cpu().numpy(),
            None if st is None else tuple(st.cpu().tolist()))


def _assert_device_equals_numpy(mf, Cur, P, GP, N, GN, thr, window=None, what=None, **kw):
    out, wmap, st = _device_filter(mf, Cur, P, GP, N, GN, thr, window, **kw)
    exp = np_temporal_filter(Cur, P, GP, N, GN, thr, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert out is None or np.array_equal(out, exp[0]), tag
    assert wmap is None or np.array_equal(wmap, exp[1]), tag
    assert st is None or st == exp[2], tag
    return exp


@pytest.mark.parametrize("name", list(CASES))
def test_temporal_filter_equals_numpy_on_the_oracles_fields(bbme, oracle, name):
    import torch
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    fwd, bwd = oracle_grids(bbme, oracle, name)
    mf = bbme.MF(f1, f2, search, block, upsample=up)
    mf.estimate_bidirectional_async()
    I1, I2 = mf.get_level_planes(0)
    assert np.array_equal(mf.get_cells(), fwd) and np.array_equal(mf.get_backward_cells(), bwd)
    CH, CW = mf.cells_shape
    odd = _odd_window(mf)
    # the context's own frames: image 1 with its next neighbour, image 2 with its previous one
    own = [(I1, None, None, I2, fwd), (I2, I1, bwd, None, None)]
    for thr in (1, 64, 1021):
        for which in (0, 1):
            assert np.array_equal(mf.temporal_filter(thr, which), np_temporal_filter(*own[which], thr)[0]), (thr, which)
        for win, np_win in ((None, mf.default_cell_window()), ("all", None), (odd, odd)):
            got = mf.temporal_filter_stats(thr, win)
            assert [_stats(g) for g in got] == [np_temporal_filter(*own[which], thr, np_win)[2] for which in (0, 1)], (thr, win)
    # the same through the entry point that takes any planes and grids
    _assert_device_equals_numpy(mf, *own[0], 64, what="image 1, oracle grid")
    _assert_device_equals_numpy(mf, *own[1], 64, odd, "image 2, oracle grid")
    _assert_device_equals_numpy(mf, I2, I1, bwd, I1, bwd, 64, odd, "image 2 between two copies of image 1", pitch_extra=3)
    _assert_device_equals_numpy(mf, I2, I1, bwd, I1, bwd, 1021, what="pitch + 1", pitch_extra=1)
    _assert_device_equals_numpy(mf, I2, I1, bwd, I1, bwd, 1, what="side stream", stream=torch.cuda.Stream())
    rng = np.random.default_rng(len(name))
    gp, gn = random_grids(CH, CW, rng, reach=2)
    _assert_device_equals_numpy(mf, I1, I2, gp, I2, gn, 64, odd, "random grids", pitch_extra=2)
    _assert_device_equals_numpy(mf, I1, I2, gp, None, None, 1021, what="random grids, previous only")
    _assert_device_equals_numpy(mf, I1, None, None, I2, gn, 1021, what="random grids, next only")
    _assert_device_equals_numpy(mf, I1, I2, gp, I2, gn, 255, what="random grids, frame only", want=("out",))
    _assert_device_equals_numpy(mf, I1, I2, gp, I2, gn, 1021, what="random grids, map only", want=("map",))
    _assert_device_equals_numpy(mf, I1, I2, gp, I2, gn, 64, odd, "random grids, statistics only", want=("stats",))
    gp, gn = extreme_grids(CH, CW, rng)
    for thr in (1, 64, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, I1, I2, gp, I2, gn, thr, what="int16 extremes")
        assert np.array_equal(out, I1) and not wmap.any() and st == (0, 0, 0, 0)
    # the injected planes and grids left the context's own alone
    assert np.array_equal(mf.temporal_filter(64), np_temporal_filter(*own[0], 64)[0])
    mf.close()


# W0 = 4 (mod 8): the last run of a cell row holds 2 cells (see tests/test_gpu_interpolation.py: only one-level contexts have such rows)
@pytest.mark.parametrize("w,h,search,block", [(132, 100, [12], [2]), (132, 100, [12], [4]), (140, 98, [12], [2])])
def test_cell_rows_that_end_inside_a_run(bbme, w, h, search, block):
    f1, f2, _ = bbme.synth_pair(w, h, 700 + w, max_motion=3)
    mf = bbme.MF(f1, f2, search, block)
    assert (mf.padded_width, mf.padded_height) == (w, h)
    CH, CW = mf.cells_shape
    assert CW % 4 != 0
    I1, I2 = mf.get_level_planes(0)
    rng = np.random.default_rng(w)
    gp, gn = random_grids(CH, CW, rng, reach=2)
    win = (CW - 7, 2, 7, CH - 5)                           # reaches the cut run
    _assert_device_equals_numpy(mf, I1, I2, gp, I2, gn, 255, win, "cut run")
    _assert_device_equals_numpy(mf, I1, None, None, I2, gn, 1021, what="cut run, next only", pitch_extra=1)
    _assert_device_equals_numpy(mf, I1, I2, gp, None, None, 64, what="cut run, odd pitch", pitch_extra=3)
    mf.estimate_bidirectional_async()
    fwd, bwd = mf.get_cells(), mf.get_backward_cells()
    for which, args in enumerate(((I1, None, None, I2, fwd), (I2, I1, bwd, None, None))):
        exp = np_temporal_filter(*args, 64)
        assert np.array_equal(mf.temporal_filter(64, which), exp[0])
        assert _stats(mf.temporal_filter_stats(64, "all")[which]) == exp[2]
    mf.close()


@pytest.fixture(scope="module")
def table_context(bbme):
    """A one-level 132 x 100 context: the division tables are injected as tensors, its own frames do not matter."""
    z = np.zeros((100, 132), np.uint8)
    mf = bbme.MF(z, z, [12], [2])
    assert (mf.padded_width, mf.padded_height) == (132, 100)
    yield mf
    mf.close()


@pytest.mark.parametrize("thr", THRS)
def test_division_by_the_strength_is_exact_in_the_kernel(table_context, thr):
    mf = table_context
    Cur, N, cost = thr_table_planes()                      # 92 x 92 inside the 132 x 100 plane; the rest is 0 against 0: weight 8
    H0, W0 = mf.padded_height, mf.padded_width
    CH, CW = mf.cells_shape
    z = np.zeros((CH, CW, 2), np.int16)
    exp = np.full((CH, CW), 8, np.int64)
    exp[:cost.shape[0], :cost.shape[1]] = thr_table_expected(cost, thr)
    _, wmap, _ = _device_filter(mf, _embed(Cur, H0, W0), None, None, _embed(N, H0, W0), z, thr, want=("map",))
    assert np.array_equal(wmap >> 4, exp) and not (wmap & 0x0f).any()
    _, wmap, _ = _device_filter(mf, _embed(Cur, H0, W0), _embed(N, H0, W0), z, None, None, thr, want=("map",))
    assert np.array_equal(wmap, exp)


def test_division_by_the_weight_sum_is_exact_in_the_kernel(table_context):
    mf = table_context
    Cur, P, N, expect_w = s_table_planes()                 # 132 x 100, the context's own size
    assert Cur.shape == (mf.padded_height, mf.padded_width)
    z = np.zeros(expect_w.shape[:2] + (2,), np.int16)
    out, wmap, _ = _device_filter(mf, Cur, P, z, N, z, 64)
    s_table_check(Cur, P, N, expect_w, out, wmap)
    Cur, P, N, expect_w = s23_table_planes()               # S = 23 with all of its 23 classes, at thr = 1021
    out, wmap, _ = _device_filter(mf, Cur, P, z, N, z, S23_THR)
    s_table_check(Cur, P, N, expect_w, out, wmap, pairs=[(8, 7)], ends=False)


def test_chain_filters_every_slot_and_batch_one_side(bbme):
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    chain = bbme.MFChain(video, search, block)
    chain.estimate_bidirectional_async()
    planes = [chain.get_slot_plane(0, s) for s in range(4)]
    fwd = [chain.get_pair_cells(p) for p in range(3)]
    bwd = [chain.get_pair_backward_cells(p) for p in range(3)]
    win = _odd_window(chain)

    def rule(f, thr, window=None):
        return np_temporal_filter(planes[f], planes[f - 1] if f > 0 else None, bwd[f - 1] if f > 0 else None,
                                  planes[f + 1] if f < 3 else None, fwd[f] if f < 3 else None, thr, window)

    for thr in (64, 1021):
        exp = [rule(f, thr)[0] for f in range(4)]
        run = chain.temporal_filter_run(thr)
        assert run.shape == (4,) + planes[0].shape
        for f in range(4):
            assert np.array_equal(run[f], exp[f]), (thr, f)
        assert np.array_equal(chain.temporal_filter_run(thr, 1, 2), np.stack(exp[1:3]))
        assert np.array_equal(chain.temporal_filter_run(thr, 3, 1)[0], exp[3])
        for p in range(3):
            assert np.array_equal(chain.get_frame_filtered(p, 0, thr), exp[p]), (thr, p)
            assert np.array_equal(chain.get_frame_filtered(p, 1, thr), exp[p + 1]), (thr, p)      # (p, 1) and (p + 1, 0): one frame
        assert np.array_equal(chain.temporal_filter(thr), exp[0])
        for w, np_win in ((None, chain.default_cell_window()), ("all", None), (win, win)):
            assert [_stats(s) for s in chain.temporal_filter_stats(thr, w)] == [rule(f, thr, np_win)[2] for f in range(4)], (thr, w)
    inner = rule(1, 64)
    assert (inner[1] & 0x0f).any() and (inner[1] >> 4).any()                       # inner frames take from both sides
    for p, w in ((0, 0), (1, 1), (2, 1)):                                          # bbme_frame_plane_device, any kind of context
        assert np.array_equal(chain.frame_plane_tensor(p, w).cpu().numpy(), planes[p + w])
    assert np.array_equal(chain.cells_tensor(1).cpu().numpy(), fwd[1])
    assert np.array_equal(chain.backward_cells_tensor(2).cpu().numpy(), bwd[2])
    chain.close()
    # a batch of the same pairs: every frame one-sided, as single contexts give it
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(3)], search, block)
    batch.estimate_bidirectional_async()
    singles = []
    for p in range(3):
        mf = bbme.MF(video[p], video[p + 1], search, block)
        mf.estimate_bidirectional_async()
        singles.append((mf.temporal_filter(64, 0), mf.temporal_filter(64, 1), mf.temporal_filter_stats(64, win)))
        assert np.array_equal(singles[p][0], np_temporal_filter(planes[p], None, None, planes[p + 1], fwd[p], 64)[0])
        assert np.array_equal(singles[p][1], np_temporal_filter(planes[p + 1], planes[p], bwd[p], None, None, 64)[0])
        a, b = mf.get_level_planes(0)
        assert np.array_equal(mf.frame_plane_tensor(0, 0).cpu().numpy(), a) and np.array_equal(mf.frame_plane_tensor(0, 1).cpu().numpy(), b)
        mf.close()
    for p in range(3):
        assert np.array_equal(batch.get_frame_filtered(p, 0, 64), singles[p][0]), p
        assert np.array_equal(batch.get_frame_filtered(p, 1, 64), singles[p][1]), p
        assert np.array_equal(batch.frame_plane_tensor(p, 1).cpu().numpy(), planes[p + 1])
    assert batch.temporal_filter_stats(64, win) == [s for single in singles for s in single[2]]
    batch.close()


def _assert_state_errors(bbme, ctx, what):
    from blockbasedmotionestimation_amd import _capi
    calls = [lambda: ctx.temporal_filter(64), lambda: ctx.temporal_filter(64, 1), lambda: ctx.temporal_filter_stats(64)]
    if isinstance(ctx, bbme.MFChain):
        calls.append(lambda: ctx.temporal_filter_run(64))
    for call in calls:
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == _capi.ERR_STATE, what


def test_temporal_filter_needs_a_valid_pair_of_fields(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    mf = bbme.MF(video[0], video[1], search, block)
    _assert_state_errors(bbme, mf, "before any estimate")
    out = torch.zeros((mf.padded_height, mf.padded_width), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    op = C.c_void_p(out.data_ptr())
    assert L.bbme_temporal_filter_device(mf._ctx, 0, 0, 64, op, mf.padded_width, None) == _capi.ERR_STATE
    assert L.bbme_temporal_filter_chain_device(mf._ctx, 0, 1, 64, op, mf.padded_width, 0, None) == _capi.ERR_UNSUPPORTED
    mf.estimate_bidirectional_async()
    first = mf.temporal_filter(64)
    assert L.bbme_temporal_filter_device(mf._ctx, 0, 0, 64, op, mf.padded_width, None) == 0
    mf.synchronize()
    assert np.array_equal(out.cpu().numpy(), first)
    mf.set_frames(video[0], video[1])
    _assert_state_errors(bbme, mf, "after a frame setter")
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter(64), first)
    mf.estimate_async()
    _assert_state_errors(bbme, mf, "after bbme_estimate")
    mf.close()
    # the entry point that takes planes and grids needs neither frames nor fields
    ctx = C.c_void_p()
    params = _capi.make_params(search, block)
    assert L.bbme_create(C.byref(params), VIDEO[0], VIDEO[1], 0, C.byref(ctx)) == 0
    z = torch.zeros((out.shape[0] // 2, out.shape[1] // 2, 2), dtype=torch.int16, device="cuda")
    cur = torch.full_like(out, 9)
    torch.cuda.synchronize()
    assert L.bbme_cells_temporal_filter_device(ctx, None, C.c_void_p(cur.data_ptr()), C.c_void_p(cur.data_ptr()), None,
                                               C.c_void_p(z.data_ptr()), 64, None, op, out.shape[1], None, 0, None, None) == 0
    assert L.bbme_synchronize(ctx) == 0
    assert bool((out == 9).all())
    assert L.bbme_temporal_filter_device(ctx, 0, 0, 64, op, out.shape[1], None) == _capi.ERR_STATE
    assert L.bbme_destroy(ctx) == 0
    # an unset chain slot
    chain = bbme.MFChain(video[:3], search, block)
    chain.estimate_bidirectional_async()
    chain.temporal_filter_run(64)
    chain.advance([video[3]])
    _assert_state_errors(bbme, chain, "between advance and the last slot")
    chain.set_frame_run(2, [video[3]])
    _assert_state_errors(bbme, chain, "slots set, not estimated")
    chain.close()


def test_temporal_filter_changes_no_state_and_refuses_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    mf = bbme.MFChain(video[:3], search, block)
    mf.estimate_bidirectional_async()

    def state():
        return dict(flow=mf.get_pair_flow(1), cells=mf.get_pair_cells(0), back=mf.get_pair_backward_cells(1),
                    fb=mf.consistency_stats_all("forward", 1), half=mf.get_pair_interpolated(1), ip=mf.interpolation_stats_all(1, 3))

    before = state()
    CH, CW = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    planes = [mf.frame_plane_tensor(p, w).clone() for p, w in ((0, 0), (0, 1), (1, 1))]
    gp, gn = mf.backward_cells_tensor(0).clone(), mf.cells_tensor(1).clone()
    out = torch.zeros((3, H0, W0), dtype=torch.uint8, device="cuda")
    wmap = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    run = mf.temporal_filter_run(64)
    stats = mf.temporal_filter_stats(64, "all")
    mf.cells_temporal_filter_device(planes[1], planes[0], planes[2], gp, gn, 64, out=out[0], weights=wmap, stats=st)
    mf.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), run[1]) and tuple(st.cpu().tolist()) == _stats(stats[1])
    # the other getters' scratch buffers and the filter's are independent
    mf.get_pair_motion_compensated(0)
    mf.compensation_errors()
    mf.get_pair_interpolated(0)
    assert np.array_equal(mf.temporal_filter_run(64), run) and mf.temporal_filter_stats(64, "all") == stats
    after = state()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    buf = np.zeros((H0, W0), np.uint8)
    s12 = (C.c_ulonglong * 12)()
    c_, p_, n_, gp_, gn_, o_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (planes[1], planes[0], planes[2], gp, gn, out, wmap, st))

    def cells(p=p_, c=c_, n=n_, a=gp_, b=gn_, thr=64, win=None, o=o_, op=W0, m=m_, mp=CW, s=s_):
        return L.bbme_cells_temporal_filter_device(ctx, p, c, n, a, b, thr, win, o, op, m, mp, s, None)

    def own(pair=0, which=0, thr=64, o=o_, op=W0):
        return L.bbme_temporal_filter_device(ctx, pair, which, thr, o, op, None)

    def run_of(first=0, count=3, thr=64, o=o_, op=W0, os=H0 * W0):
        return L.bbme_temporal_filter_chain_device(ctx, first, count, thr, o, op, os, None)

    def host(pair=0, which=0, thr=64, o=buf.ctypes.data):
        return L.bbme_get_temporal_filtered_host(ctx, pair, which, thr, o)

    assert cells() == 0 and own() == 0 and run_of() == 0 and host() == 0
    assert cells(p=None, a=None) == 0 and cells(n=None, b=None) == 0
    assert cells(p=None, a=None, n=None, b=None) == inv                          # no neighbour at all
    assert cells(p=None) == inv and cells(a=None) == inv and cells(n=None) == inv and cells(b=None) == inv
    assert cells(c=None) == inv
    assert cells(o=None, m=None, s=None) == inv                                  # nothing asked for
    for plane in (c_, p_, n_):                                                   # an output inside an input plane
        assert cells(o=plane) == inv
    assert cells(o=C.c_void_p(c_.value + W0), op=W0) == inv and cells(n=None, b=None, o=n_) == 0
    assert cells(o=None) == 0 and cells(m=None) == 0 and cells(s=None) == 0 and cells(o=None, m=None) == 0
    assert own(o=None) == inv and run_of(o=None) == inv and host(o=None) == inv
    assert L.bbme_temporal_filter_stats(ctx, 64, None, None) == inv
    for thr in (0, -5, 1022):
        assert cells(thr=thr) == inv and own(thr=thr) == inv and run_of(thr=thr) == inv and host(thr=thr) == inv, thr
        assert L.bbme_temporal_filter_stats(ctx, thr, None, s12) == inv
    for pair in (-1, 2):
        assert own(pair=pair) == inv and host(pair=pair) == inv
    for which in (-1, 2):
        assert own(which=which) == inv and host(which=which) == inv
    for first, count in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (1, -1)):
        assert run_of(first=first, count=count) == inv, (first, count)
    assert run_of(first=2, count=1) == 0 and run_of(first=1, count=2) == 0
    assert cells(op=W0 - 1) == inv and own(op=W0 - 1) == inv and run_of(op=W0 - 1) == inv
    assert cells(mp=CW - 1) == inv
    assert cells(mp=CW - 1, m=None) == 0 and cells(op=W0 - 1, o=None) == 0       # a pitch of nothing is not looked at
    assert run_of(count=2, os=H0 * W0 - 1) == inv
    assert run_of(count=1, os=0) == 0                                            # one frame has no stride
    for win in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (CW - 7, 0, 8, 8), (0, CH - 7, 8, 8), (0, 0, CW + 1, CH)):
        w4 = (C.c_int * 4)(*win)
        assert cells(win=w4) == inv, win
        assert L.bbme_temporal_filter_stats(ctx, 64, w4, s12) == inv, win
    assert L.bbme_temporal_filter_stats(ctx, 64, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s12) == 0
    pp = C.c_void_p()
    assert L.bbme_frame_plane_device(ctx, 0, 0, 0, None) == inv
    for pair, which, level in ((-1, 0, 0), (2, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 3), (0, 0, -1)):
        assert L.bbme_frame_plane_device(ctx, pair, which, level, C.byref(pp)) == inv, (pair, which, level)
    assert L.bbme_frame_plane_device(ctx, 1, 1, 2, C.byref(pp)) == 0 and pp.value
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_device(planes[1], planes[0], None, gp[:, :CW - 2], None, 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.temporal_filter_run(64, 2, 3)
    assert e.value.status == inv
    mf.synchronize()
    after = state()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    assert np.array_equal(mf.temporal_filter_run(64), run)
    mf.close()


@pytest.fixture(scope="module")
def denoise_reference(bbme):
    """7 frames of the video and, per frame, the rule on (previous, current, next) with the fields of single MF contexts."""
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(VIDEO[0], VIDEO[1], 7, VIDEO[3], max_motion=VIDEO[4])
    planes, fwd, bwd = [None] * 7, [None] * 6, [None] * 6
    for p in range(6):
        mf = bbme.MF(video[p], video[p + 1], search, block)
        mf.estimate_bidirectional_async()
        planes[p], planes[p + 1] = mf.get_level_planes(0)
        fwd[p], bwd[p] = mf.get_cells(), mf.get_backward_cells()
        px, py = mf.padding_x, mf.padding_y
        mf.close()
    exp = []
    for f in range(7):
        full = np_temporal_filter(planes[f], planes[f - 1] if f > 0 else None, bwd[f - 1] if f > 0 else None,
                                  planes[f + 1] if f < 6 else None, fwd[f] if f < 6 else None, 96)[0]
        exp.append(full[py:py + VIDEO[1], px:px + VIDEO[0]])
    return video, exp


@pytest.mark.parametrize("in_flight,batch", [(4, 2), (1, 1)])
def test_denoise_frames(bbme, denoise_reference, in_flight, batch):
    """in_flight=4, batch=2: two contexts, a carried round each and the segment boundary at frame 3."""
    from blockbasedmotionestimation_amd.sequence import denoise_frames
    search, block = VIDEO_PARAMS
    video, exp = denoise_reference
    keep = [v.copy() for v in video]
    got = denoise_frames(video, search, block, 96, in_flight=in_flight, batch=batch)
    assert len(got) == 7
    for v, k in zip(video, keep):
        assert np.array_equal(v, k)
    for f in range(7):
        assert got[f].shape == (VIDEO[1], VIDEO[0]) and got[f].dtype == np.uint8
        assert np.array_equal(got[f], exp[f]), f
    assert any(not np.array_equal(got[f], video[f]) for f in range(7))
    assert len(denoise_frames(video[:1], search, block, 96)) == 1


def test_cli_writes_the_denoised_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    f1, f2, _ = bbme.synth_pair(96, 72, 1001, max_motion=3)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    base = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm"), "--levels", "3", "--block", "16", "--search", "30"]
    r = subprocess.run(base + ["--no-upsample", "--denoise", str(tmp_path / "dn"), "--strength", "96"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    px, py = mf.padding_x, mf.padding_y
    for which in (0, 1):
        frame = mf.temporal_filter(96, which)[py:py + 72, px:px + 96]
        assert (tmp_path / ("dn_%d.pgm" % (which + 1))).read_bytes() == b"P5\n96 72\n255\n" + frame.tobytes(), which
    mf.close()
    r = subprocess.run(base + ["--denoise", str(tmp_path / "up")], capture_output=True, text=True)
    assert r.returncode == 2 and "--no-upsample" in r.stderr
    assert not (tmp_path / "up_1.pgm").exists()
    r = subprocess.run(base + ["--no-upsample", "--denoise", str(tmp_path / "bad"), "--strength", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--denoise" in r.stderr
