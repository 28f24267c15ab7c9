"""Motion-compensated interpolation on the GPU (include/bbme.h, "INTERPOLATION RULE"): k_interpolate gives exactly the numpy
restatement of the rule (test_interpolation_cpu.np_interpolate) on the oracle's two grids and the context's level-0 planes, on
injected grids (random, int16 extremes, no backward grid), with windows, caller pitches that are not multiples of 4, side streams
and geometries whose cell rows end inside a lane's run; batches and chains equal single contexts; the blend's division is exact
for every numerator; the calls change no context state and refuse bad arguments."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _odd_window, _stats_of, _write_pgm
from test_gpu_bidirectional import CASES, _frames
from test_interpolation_cpu import (DIVISION_DENS, STAT_KEYS, extreme_grids, np_interpolate, oracle_grids, ramp_expected,
                                    ramp_pair, random_grids)

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

VIDEO = (200, 136, 4, 77, 6)                               # synth_video(width, height, frames, seed, max_motion=...)
VIDEO_PARAMS = ([30, 30, 30], [16, 16, 16])


def _device_interpolate(mf, f, b, num0, count, den, window=None, pitch_extra=0, stream=None, want=("out", "sel", "stats")):
    """cells_interpolate_device on host grids -> (frames (count, H0, W0), maps (count, CH, CW), [stats tuples]) as numpy / lists,
    None where not asked for; rows of both outputs are pitch_extra bytes further apart than packed."""
    import torch
    CH, CW = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    tf = torch.from_numpy(np.ascontiguousarray(f)).cuda()
    tb = None if b is None else torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((count, H0, W0 + pitch_extra), 0xAA, dtype=torch.uint8, device="cuda") if "out" in want else None
    sel = torch.full((count, CH, CW + pitch_extra), 0xAA, dtype=torch.uint8, device="cuda") if "sel" in want else None
    st = torch.zeros((count, 4), dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    mf.cells_interpolate_device(tf, tb, num0, count, den, out=None if out is None else out[:, :, :W0],
                                sel=None if sel is None else sel[:, :, :CW], stats=st, window=window,
                                hip_stream_handle=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    if pitch_extra:                                        # the bytes between the rows stay untouched
        assert out is None or bool((out[:, :, W0:] == 0xAA).all())
        assert sel is None or bool((sel[:, :, CW:] == 0xAA).all())
    return (None if out is None else out[:, :, :W0].cpu().numpy(), None if sel is None else sel[:, :, :CW].cpu().numpy(),
            None if st is None else [tuple(r) for r in st.cpu().tolist()])


def _assert_device_equals_numpy(mf, I1, I2, f, b, num0, count, den, window=None, what=None, **kw):
    out, sel, st = _device_interpolate(mf, f, b, num0, count, den, window, **kw)
    for q in range(count):
        exp = np_interpolate(I1, I2, f, b, num0 + q, den, window)
        tag = (what, num0 + q, den, b is not None, window)
        assert out is None or np.array_equal(out[q], exp[0]), tag
        assert sel is None or np.array_equal(sel[q], exp[1]), tag
        assert st is None or st[q] == exp[2], tag


@pytest.mark.parametrize("name", list(CASES))
def test_interpolation_equals_numpy_on_the_oracles_fields(bbme, oracle, name):
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
    for num, den in ((1, 2), (1, 3), (2, 3)):
        exp = np_interpolate(I1, I2, fwd, bwd, num, den, mf.default_cell_window())
        assert np.array_equal(mf.interpolate(num, den), exp[0]), (num, den)
        assert _stats(mf.interpolation_stats(num, den)) == exp[2], (num, den)
        assert _stats(mf.interpolation_stats(num, den, "all")) == np_interpolate(I1, I2, fwd, bwd, num, den)[2], (num, den)
        assert _stats(mf.interpolation_stats(num, den, odd)) == np_interpolate(I1, I2, fwd, bwd, num, den, odd)[2], (num, den)
    run = mf.interpolate_run(4)
    assert run.shape == (3, 2 * CH, 2 * CW)
    for num in (1, 2, 3):
        assert np.array_equal(run[num - 1], np_interpolate(I1, I2, fwd, bwd, num, 4)[0]), num
    # the same through the entry point that takes any two grids
    _assert_device_equals_numpy(mf, I1, I2, fwd, bwd, 1, 3, 4, what="oracle grids, run of 4")
    _assert_device_equals_numpy(mf, I1, I2, fwd, bwd, 1, 1, 2, odd, "odd window")
    _assert_device_equals_numpy(mf, I1, I2, fwd, None, 2, 1, 3, what="no backward grid")
    _assert_device_equals_numpy(mf, I1, I2, fwd, bwd, 1, 2, 3, odd, "pitch not a multiple of 4", pitch_extra=3)
    _assert_device_equals_numpy(mf, I1, I2, fwd, bwd, 1, 1, 2, what="pitch + 1", pitch_extra=1)
    _assert_device_equals_numpy(mf, I1, I2, fwd, bwd, 2, 2, 5, what="side stream", stream=torch.cuda.Stream())
    rng = np.random.default_rng(len(name))
    f, b = random_grids(CH, CW, rng)
    _assert_device_equals_numpy(mf, I1, I2, f, b, 1, 2, 3, odd, "random grids", pitch_extra=2)
    _assert_device_equals_numpy(mf, I1, I2, f, None, 254, 2, 256, what="random grids, no backward grid")
    _assert_device_equals_numpy(mf, I1, I2, f, b, 127, 2, 255, what="random grids, den 255", want=("out",))
    _assert_device_equals_numpy(mf, I1, I2, f, b, 1, 1, 2, what="random grids, map only", want=("sel",))
    _assert_device_equals_numpy(mf, I1, I2, f, b, 3, 1, 5, odd, "random grids, statistics only", want=("stats",))
    f, b = extreme_grids(CH, CW, rng)
    for num, den in ((1, 2), (1, 256), (255, 256), (2, 3)):
        _assert_device_equals_numpy(mf, I1, I2, f, b, num, 1, den, what="int16 extremes")
    _, sel, st = _device_interpolate(mf, f, b, 1, 1, 2)
    assert (sel == 2).all() and st[0][:3] == (0, 0, CH * CW)
    # the injected grids left the context's own fields alone
    assert np.array_equal(mf.interpolate(1, 2), np_interpolate(I1, I2, fwd, bwd, 1, 2)[0])
    mf.close()


# W0 = 4 (mod 8): the last run of a cell row holds 2 cells.  A context needs every level's width to be a multiple of 4, so with two
# levels W0 is a multiple of 8 (132 x 100 with blocks [2, 2] is refused: level 1 would be 66 wide) and only one-level contexts have
# such a row; none has an odd number of cells per row (the host rule takes one in tests/test_interpolation_cpu.py).
@pytest.mark.parametrize("w,h,search,block", [(132, 100, [12], [2]), (132, 100, [12], [4]), (140, 98, [12], [2])])
def test_cell_rows_that_end_inside_a_run(bbme, w, h, search, block):
    f1, f2, _ = bbme.synth_pair(w, h, 700 + w, max_motion=3)
    mf = bbme.MF(f1, f2, search, block)
    assert (mf.padded_width, mf.padded_height) == (w, h)
    CH, CW = mf.cells_shape
    assert CW % 4 != 0
    I1, I2 = mf.get_level_planes(0)
    rng = np.random.default_rng(w)
    f, b = random_grids(CH, CW, rng)
    win = (CW - 7, 2, 7, CH - 5)                           # reaches the cut run
    _assert_device_equals_numpy(mf, I1, I2, f, b, 1, 2, 3, win, "cut run")
    _assert_device_equals_numpy(mf, I1, I2, f, None, 1, 1, 2, what="cut run, no backward grid", pitch_extra=1)
    _assert_device_equals_numpy(mf, I1, I2, f, b, 3, 1, 4, what="cut run, odd pitch", pitch_extra=3)
    mf.estimate_bidirectional_async()
    exp = np_interpolate(I1, I2, mf.get_cells(), mf.get_backward_cells(), 1, 2)
    assert np.array_equal(mf.interpolate(), exp[0]) and _stats(mf.interpolation_stats(1, 2, "all")) == exp[2]
    mf.close()


def test_batch_and_chain_equal_single_contexts(bbme):
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    singles = []
    for p in range(3):
        mf = bbme.MF(video[p], video[p + 1], search, block)
        mf.estimate_bidirectional_async()
        win = _odd_window(mf)
        singles.append(dict(half=mf.interpolate(1, 2), third=mf.interpolate(2, 3), run=mf.interpolate_run(3),
                            stats=mf.interpolation_stats(1, 2), stats_all=mf.interpolation_stats(2, 3, "all"),
                            stats_odd=mf.interpolation_stats(1, 4, win)))
        I1, I2 = mf.get_level_planes(0)
        exp = np_interpolate(I1, I2, mf.get_cells(), mf.get_backward_cells(), 1, 2, mf.default_cell_window())
        assert np.array_equal(singles[p]["half"], exp[0]) and _stats(singles[p]["stats"]) == exp[2]
        assert all(exp[2][k] > 0 for k in range(4)), exp[2]                         # every hypothesis is selected somewhere
        mf.close()
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(3)], search, block)
    chain = bbme.MFChain(video, search, block)
    for ctx, what in ((batch, "batch"), (chain, "chain")):
        ctx.estimate_bidirectional_async()
        assert ctx.interpolation_stats_all(1, 2) == [s["stats"] for s in singles], what
        assert ctx.interpolation_stats_all(2, 3, "all") == [s["stats_all"] for s in singles], what
        assert ctx.interpolation_stats_all(1, 4, win) == [s["stats_odd"] for s in singles], what
        for p in range(3):
            assert np.array_equal(ctx.get_pair_interpolated(p), singles[p]["half"]), (what, p)
            assert np.array_equal(ctx.get_pair_interpolated(p, 2, 3), singles[p]["third"]), (what, p)
            assert np.array_equal(ctx.interpolate_run(3, pair=p), singles[p]["run"]), (what, p)
        assert np.array_equal(ctx.interpolate(1, 2), singles[0]["half"]), what       # the inherited call addresses pair 0
        ctx.close()


def test_direction_backward_exchanges_the_planes(bbme):
    name = "cfg1_like"
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    mf = bbme.MF(f1, f2, search, block, upsample=up)
    mf.estimate_bidirectional_async()
    f, b = mf.get_cells(), mf.get_backward_cells()
    I1, I2 = mf.get_level_planes(0)
    mf.set_direction(True)
    a1, a2 = mf.get_level_planes(0)                            # the accessors stay physical
    assert np.array_equal(a1, I1) and np.array_equal(a2, I2)
    _assert_device_equals_numpy(mf, I2, I1, b, f, 1, 2, 3, what="backward")
    _assert_device_equals_numpy(mf, I2, I1, b, None, 1, 1, 4, _odd_window(mf), "backward, no second grid")
    mf.set_direction(False)
    _assert_device_equals_numpy(mf, I1, I2, f, b, 2, 1, 3, what="forward again")
    # a chain context in direction BACKWARD: pair p reads slot p + 1 as its image 1
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    chain = bbme.MFChain(video[:3], search, block)
    chain.set_direction(True)
    rng = np.random.default_rng(9)
    g, h = random_grids(*chain.cells_shape, rng)
    px, py = chain.padding_x, chain.padding_y
    planes = [bbme.pad_zero(v, px, py) for v in video[:3]]
    import torch
    tg, th = torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()
    out = torch.zeros((1,) + planes[0].shape, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for p in range(2):
        chain.cells_interpolate_device(tg, th, 1, 1, 2, pair=p, out=out)
        chain.synchronize()
        assert np.array_equal(out[0].cpu().numpy(), np_interpolate(planes[p + 1], planes[p], g, h, 1, 2)[0]), p
    chain.close()
    mf.close()


def test_every_numerator_meets_the_exact_quotient_in_the_kernel(bbme):
    import torch
    I1, I2 = ramp_pair()
    mf = bbme.MF(I1, I2, [32], [16])
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == (256, 256, 0, 0)
    p1, p2 = mf.get_level_planes(0)
    assert np.array_equal(p1, I1) and np.array_equal(p2, I2)
    z = torch.zeros((128, 128, 2), dtype=torch.int16, device="cuda")
    for den in DIVISION_DENS:
        out = torch.zeros((den - 1, 256, 256), dtype=torch.uint8, device="cuda")
        sel = torch.ones((den - 1, 128, 128), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        mf.cells_interpolate_device(z, z if den % 2 else None, 1, den - 1, den, out=out, sel=sel)      # one launch per den
        mf.synchronize()
        got = out.cpu().numpy()
        for num in range(1, den):
            assert np.array_equal(got[num - 1], ramp_expected(num, den)), (num, den)
        assert not bool(sel.any())
    mf.close()


def _assert_state_errors(bbme, ctx, what):
    from blockbasedmotionestimation_amd import _capi
    for call in (lambda: ctx.interpolate(1, 2), lambda: ctx.interpolate_run(2), lambda: ctx.interpolation_stats(1, 2)):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == _capi.ERR_STATE, what


def test_interpolation_needs_a_valid_pair_of_fields(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    mf = bbme.MF(video[0], video[1], search, block)
    _assert_state_errors(bbme, mf, "before any estimate")
    mf.estimate_bidirectional_async()
    half = mf.interpolate()
    mf.set_frames(video[0], video[1])
    _assert_state_errors(bbme, mf, "after a frame setter")
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.interpolate(), half)
    mf.estimate_async()
    _assert_state_errors(bbme, mf, "after bbme_estimate")
    # the entry point that takes grids needs frames, not fields
    CH, CW = mf.cells_shape
    z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    out = torch.zeros((1, mf.padded_height, mf.padded_width), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    mf.cells_interpolate_device(z, None, 1, 1, 2, out=out)
    mf.synchronize()
    mf.close()
    # a context without frames
    ctx = C.c_void_p()
    params = _capi.make_params(search, block)
    assert L.bbme_create(C.byref(params), VIDEO[0], VIDEO[1], 0, C.byref(ctx)) == 0
    zp, op = C.c_void_p(z.data_ptr()), C.c_void_p(out.data_ptr())
    assert L.bbme_cells_interpolate_device(ctx, 0, zp, None, 1, 1, 2, None, op, mf.padded_width, 0, None, 0, 0, None, None) == _capi.ERR_STATE
    assert L.bbme_interpolate_device(ctx, 0, 1, 1, 2, op, mf.padded_width, 0, None) == _capi.ERR_STATE
    assert L.bbme_destroy(ctx) == 0
    # an unset chain slot
    chain = bbme.MFChain(video[:3], search, block)
    chain.estimate_bidirectional_async()
    chain.get_pair_interpolated(1)
    chain.advance([video[3]])
    _assert_state_errors(bbme, chain, "between advance and the last slot")
    with pytest.raises(bbme.BbmeError) as e:
        chain.cells_interpolate_device(z, None, 1, 1, 2, out=out)
    assert e.value.status == _capi.ERR_STATE
    chain.set_frame_run(2, [video[3]])
    _assert_state_errors(bbme, chain, "slots set, not estimated")
    chain.cells_interpolate_device(z, None, 1, 1, 2, pair=1, out=out)
    chain.synchronize()
    chain.close()


def test_interpolation_changes_no_state_and_refuses_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    f1, f2, _ = bbme.synth_pair(200, 136, 901, max_motion=7)
    search, block = [30] * 3, [16] * 3
    mf = bbme.MF(f1, f2, search, block)
    mf.estimate_bidirectional_async()

    def state():
        return dict(flow=mf.get_flow(), cells=mf.get_cells(), back=mf.get_backward_cells(),
                    fb=mf.consistency_stats("forward", 1), fb_back=mf.consistency_stats("backward", 1, "all"))

    before = state()
    CH, CW = mf.cells_shape
    H0, W0 = mf.padded_height, mf.padded_width
    tf = torch.from_numpy(before["cells"]).cuda()
    tb = torch.from_numpy(before["back"]).cuda()
    out = torch.zeros((3, H0, W0), dtype=torch.uint8, device="cuda")
    sel = torch.zeros((3, CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    half = mf.interpolate()
    mf.interpolate_run(5)
    mf.interpolation_stats(2, 3)
    mf.cells_interpolate_device(tf, tb, 1, 3, 4, out=out, sel=sel, stats=st)
    mf.synchronize()
    assert np.array_equal(out.cpu().numpy(), mf.interpolate_run(4))
    assert [tuple(r) for r in st.cpu().tolist()] == [_stats(mf.interpolation_stats(n, 4, "all")) for n in (1, 2, 3)]
    # the other getters' scratch buffers and the interpolation's are independent
    mf.draw_MVimage()
    mf.compensation_error()
    mf.consistency("forward", 1)
    assert np.array_equal(mf.interpolate(), half)
    after = state()
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    buf = np.zeros((H0, W0), np.uint8)
    s4 = (C.c_ulonglong * 4)()
    f_, b_, o_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (tf, tb, out, sel, st))

    def cells(pair=0, f=f_, b=b_, num0=1, count=1, den=2, win=None, o=o_, op=W0, os=H0 * W0, m=m_, mp=CW, ms=CH * CW, s=s_):
        return L.bbme_cells_interpolate_device(ctx, pair, f, b, num0, count, den, win, o, op, os, m, mp, ms, s, None)

    def own(pair=0, num0=1, count=1, den=2, o=o_, op=W0, os=H0 * W0):
        return L.bbme_interpolate_device(ctx, pair, num0, count, den, o, op, os, None)

    assert cells() == 0 and own() == 0 and cells(b=None) == 0
    assert cells(count=3, den=4) == 0 and own(count=3, den=4) == 0
    for pair in (-1, 1):
        assert cells(pair=pair) == inv and own(pair=pair) == inv
        assert L.bbme_get_interpolated_host(ctx, pair, 1, 2, buf.ctypes.data) == inv
    assert cells(f=None) == inv
    assert cells(o=None, m=None, s=None) == inv                 # nothing asked for
    assert cells(o=None) == 0 and cells(m=None) == 0 and cells(s=None) == 0 and cells(o=None, m=None) == 0
    assert own(o=None) == inv
    assert L.bbme_get_interpolated_host(ctx, 0, 1, 2, None) == inv
    assert L.bbme_interpolation_stats(ctx, 1, 2, None, None) == inv
    for den in (1, 0, -3, 257):
        assert cells(den=den) == inv and own(den=den) == inv, den
        assert L.bbme_get_interpolated_host(ctx, 0, 1, den, buf.ctypes.data) == inv
        assert L.bbme_interpolation_stats(ctx, 1, den, None, s4) == inv
    for num0, count, den in ((0, 1, 2), (-1, 1, 4), (2, 1, 2), (1, 0, 4), (1, -1, 4), (1, 4, 4), (3, 2, 4), (256, 1, 256)):
        assert cells(num0=num0, count=count, den=den) == inv, (num0, count, den)
        assert own(num0=num0, count=count, den=den) == inv, (num0, count, den)
    for num, den in ((0, 2), (2, 2), (4, 3)):
        assert L.bbme_get_interpolated_host(ctx, 0, num, den, buf.ctypes.data) == inv
        assert L.bbme_interpolation_stats(ctx, num, den, None, s4) == inv
    assert cells(op=W0 - 1) == inv and own(op=W0 - 1) == inv
    assert cells(mp=CW - 1) == inv
    assert cells(mp=CW - 1, m=None) == 0 and cells(op=W0 - 1, o=None) == 0       # a pitch of nothing is not looked at
    assert cells(count=2, den=3, os=H0 * W0 - 1) == inv and own(count=2, den=3, os=H0 * W0 - 1) == inv
    assert cells(count=2, den=3, ms=CH * CW - 1) == inv
    assert cells(count=1, den=3, os=0, ms=0) == 0 and own(count=1, den=3, os=0) == 0      # one frame has no stride
    for win in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (CW - 7, 0, 8, 8), (0, CH - 7, 8, 8), (0, 0, CW + 1, CH)):
        w4 = (C.c_int * 4)(*win)
        assert cells(win=w4) == inv, win
        assert L.bbme_interpolation_stats(ctx, 1, 2, w4, s4) == inv, win
    assert L.bbme_interpolation_stats(ctx, 1, 2, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s4) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_interpolate_device(tf[:, :CW - 2], tb, 1, 1, 2, out=out[:1])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.interpolate_run(1)
    assert e.value.status == inv
    mf.synchronize()
    after = state()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    assert np.array_equal(mf.interpolate(), half)
    mf.close()


@pytest.mark.parametrize("factor", [2, 3])
def test_interpolate_frames(bbme, factor):
    from blockbasedmotionestimation_amd.sequence import interpolate_frames
    search, block = VIDEO_PARAMS
    video = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
    keep = [v.copy() for v in video]
    got = interpolate_frames(video, search, block, factor, in_flight=4, batch=2)
    assert len(got) == factor * 3 + 1
    for v, k in zip(video, keep):
        assert np.array_equal(v, k)
    for p in range(3):
        assert np.array_equal(got[factor * p], video[p]), p
        mf = bbme.MF(video[p], video[p + 1], search, block)
        mf.estimate_bidirectional_async()
        px, py = mf.padding_x, mf.padding_y
        for k in range(1, factor):
            exp = mf.interpolate(k, factor)[py:py + VIDEO[1], px:px + VIDEO[0]]
            assert got[factor * p + k].shape == (VIDEO[1], VIDEO[0])
            assert np.array_equal(got[factor * p + k], exp), (p, k)
        mf.close()
    assert np.array_equal(got[-1], video[3])
    assert len(interpolate_frames(video[:1], search, block, factor)) == 1


def test_cli_writes_the_interpolated_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    f1, f2, _ = bbme.synth_pair(96, 72, 1001, max_motion=3)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    args = ["--levels", "3", "--block", "16", "--search", "30"]
    base = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm")] + args
    r = subprocess.run(base + ["--interpolate", str(tmp_path / "mid"), "--factor", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3, upsample=4)
    mf.estimate_bidirectional_async()
    px, py, w, h = mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height
    for k in (1, 2):
        frame = mf.interpolate(k, 3)[py:py + h, px:px + w]
        assert (tmp_path / ("mid_%d.pgm" % k)).read_bytes() == b"P5\n%d %d\n255\n" % (w, h) + frame.tobytes(), k
    assert not (tmp_path / "mid_3.pgm").exists()
    mf.close()
    r = subprocess.run(base + ["--no-upsample", "--interpolate", str(tmp_path / "plain")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    px, py = mf.padding_x, mf.padding_y
    frame = mf.interpolate(1, 2)[py:py + 72, px:px + 96]
    assert (tmp_path / "plain_1.pgm").read_bytes() == b"P5\n96 72\n255\n" + frame.tobytes()
    mf.close()
    r = subprocess.run(base + ["--interpolate", str(tmp_path / "bad"), "--factor", "1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--interpolate" in r.stderr
