"""Colour interpolation at quarter-pel positions on the GPU (include/bbme.h, "BGR SUBPEL INTERPOLATION RULE"), all bit-exact:
k_subpel_interpolate_bgr gives the numpy restatement of tests/test_subpel_interpolation_bgr_cpu.py on geometries with odd
paddings and cut runs, with injected fraction and edge grids, stored and caller's colour, colour and output pitches that reach the
byte paths, strided grids, runs of phases and a side stream; the context's own calls follow its refined fields; grey frames give
the grey subpel frame in every channel; 4 x integer grids give k_interpolate_bgr's frame; batches and chains equal single
contexts; direction BACKWARD equals the exchanged pair; a grey setter withdraws the colour; nothing changes context state; guard
bands stay whole under poison; the sequence driver and the command line write the same frames."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _cuda, _status
from test_bgr_cpu import SHAPES, colour_pair, luma_planes, np_bgr_to_gray
from test_gpu_bgr import VIDEO, VIDEO_PARAMS, _device_bgr, _pitched, _write_ppm, colour_video
from test_subpel_interpolation_bgr_cpu import near_colour_pair, np_subpel_interpolate_bgr
from test_subpel_interpolation_cpu import edge_grid, fraction_grids, np_subpel_interpolate

pytestmark = pytest.mark.gpu

_cache = {}


def _device(mf, qf, qb, num0, count, den, colour=None, colour_extra=0, out_extra=0, q_extra=0, stream=None, pair=0):
    """cells_interpolate_subpel_bgr_device on host grids -> (count, H, W, 3) numpy; the grids' rows q_extra cells further apart than
    packed; colour = (c1, c2) host frames handed over as tensors whose rows are colour_extra bytes further apart than packed, None =
    the stored colour; the output's rows out_extra bytes further apart than packed: the bytes between the rows and behind the
    buffer stay untouched."""
    import torch
    h, w = mf.orig_height, mf.orig_width
    CH, CW = mf.cells_shape
    tq = []
    for q in (qf, qb):
        if q is None:
            tq.append(None)
            continue
        t = torch.full((CH, CW + q_extra, 2), 0x7777, dtype=torch.int16, device="cuda")
        t[:, :CW] = _cuda(np.asarray(q, np.int16))
        tq.append(t[:, :CW])
    t1 = t2 = None
    if colour is not None:
        t1, t2 = (torch.from_numpy(_pitched(c, 3 * w + colour_extra)).cuda().as_strided((h, w, 3), (3 * w + colour_extra, 3, 1))
                  for c in colour)
    pitch = 3 * w + out_extra
    raw = torch.full((count * h * pitch + 3,), 0xAA, dtype=torch.uint8, device="cuda")
    out = raw.as_strided((count, h, w, 3), (h * pitch, pitch, 3, 1))
    torch.cuda.synchronize()
    mf.cells_interpolate_subpel_bgr_device(tq[0], tq[1], t1, t2, num0, count, den, pair=pair, out=out,
                                           stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    rows = raw[:count * h * pitch].view(count * h, pitch)
    assert bool((rows[:, 3 * w:] == 0xAA).all()) and bool((raw[count * h * pitch:] == 0xAA).all())
    return out.cpu().numpy()


def _assert_device_equals_numpy(mf, I1, I2, c1, c2, qf, qb, num0, count, den, own, what, **kw):
    got = _device(mf, qf, qb, num0, count, den, (c1, c2) if own else None, **kw)
    px, py = mf.padding_x, mf.padding_y
    for q in range(count):
        exp = np_subpel_interpolate_bgr(I1, I2, c1, c2, qf, qb, num0 + q, den, px, py)
        assert np.array_equal(got[q], exp), (what, num0 + q, den, qb is not None, own, kw, np.argwhere(got[q] != exp)[:4])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_injected_grids_equal_numpy(bbme, shape):
    import torch
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    c1, c2 = near_colour_pair(w, h, 5 * w + h)
    mf = bbme.MF(c1, c2, list(search), list(block))
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == SHAPES[shape]
    I1, I2 = mf.get_level_planes(0)
    e1, e2 = luma_planes(c1, c2, px, py)
    assert np.array_equal(I1, e1) and np.array_equal(I2, e2)
    qf, qb = fraction_grids(H0, W0, H0 + W0)
    _, sel, _ = np_subpel_interpolate(I1, I2, qf, qb, 1, 2)
    assert set(np.unique(sel).tolist()) == {0, 1, 2}        # every hypothesis is selected somewhere
    # (num0, count, den, backward grid, caller's colour, its extra pitch, the output's extra pitch, the grids' extra pitch)
    for num0, count, den, with_b, own, c_extra, o_extra, q_extra in (
            (1, 1, 2, True, False, 0, 0, 0), (1, 3, 4, True, True, 0, 1, 3), (1, 1, 3, False, True, 1, 3, 0),
            (2, 3, 5, False, False, 0, 3, 1), (255, 1, 256, True, True, 7, 0, 3), (1, 3, 4, True, False, 0, 0, 0)):
        _assert_device_equals_numpy(mf, I1, I2, c1, c2, qf, qb if with_b else None, num0, count, den, own, "fractions",
                                    colour_extra=c_extra, out_extra=o_extra, q_extra=q_extra)
    _assert_device_equals_numpy(mf, I1, I2, c1, c2, qf, qb, 1, 2, 3, False, "side stream", stream=torch.cuda.Stream(), q_extra=3)
    # points on and past every edge
    for num, den in ((1, 2), (2, 5)):
        E, cells = edge_grid(H0, W0, num, den, 11 + den)
        assert len(cells) >= 60 and {v for _, _, v in cells} == {True, False}
        _assert_device_equals_numpy(mf, I1, I2, c1, c2, E, None, num, 1, den, False, "edges", out_extra=1)
        _assert_device_equals_numpy(mf, I1, I2, c1, c2, E, (-E).astype(np.int16), num, 1, den, True, "edges, both grids", colour_extra=1,
                                    q_extra=3)
    # the context's own fields
    mf.estimate_bidirectional_async()
    qf, qb = mf.subpel_cells("forward"), mf.subpel_cells("backward")
    assert np.array_equal(mf.interpolate_subpel_bgr(1, 2), np_subpel_interpolate_bgr(I1, I2, c1, c2, qf, qb, 1, 2, px, py))
    run = mf.interpolate_run_subpel_bgr(4)
    assert run.shape == (3, h, w, 3)
    for num in (1, 2, 3):
        assert np.array_equal(run[num - 1], np_subpel_interpolate_bgr(I1, I2, c1, c2, qf, qb, num, 4, px, py)), num
    out = np.empty((h, w, 3), np.uint8)
    assert mf.interpolate_subpel_bgr(2, 3, out=out) is out
    assert np.array_equal(out, np_subpel_interpolate_bgr(I1, I2, c1, c2, qf, qb, 2, 3, px, py))
    mf.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_edges_on_flat_luma_with_a_callers_colour(bbme, shape):
    """On flat planes (their zero border apart) the forward hypothesis is selected wherever it is valid and costs nothing, so the
    colour taps of P1 and P2 reach every edge of the frame; the colour is a caller's, random"""
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    flat = np.full((h, w), 77, np.uint8)
    mf = bbme.MF(flat, flat, list(search), list(block))
    I1, I2 = mf.get_level_planes(0)
    c1, c2 = colour_pair(w, h, 7 * w + h)
    moved = 0
    for num, den in ((1, 2), (1, 3), (3, 4)):
        E, cells = edge_grid(H0, W0, num, den, 11 + den)
        moved += int((np_subpel_interpolate(I1, I2, E, None, num, den)[1] == 0).sum())
        _assert_device_equals_numpy(mf, I1, I2, c1, c2, E, None, num, 1, den, True, "edges, flat luma", colour_extra=den - 2, out_extra=1)
    assert moved > 100
    mf.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_property_1_grey_frames_give_the_grey_subpel_frame_in_every_channel(bbme, shape):
    w, h, search, block = shape
    _, _, px, py = SHAPES[shape]
    g1, g2, _ = bbme.synth_pair(w, h, 300 + w + h, max_motion=3)
    mf = bbme.MF(np.repeat(g1[..., None], 3, 2), np.repeat(g2[..., None], 3, 2), list(search), list(block))
    mf.estimate_bidirectional_async()
    for num, den in ((1, 2), (2, 3)):
        grey = mf.interpolate_subpel(num, den)[py:py + h, px:px + w]
        got = mf.interpolate_subpel_bgr(num, den)
        for ch in range(3):
            assert np.array_equal(got[..., ch], grey), (num, den, ch)
    mf.close()


@pytest.mark.parametrize("shape", [(130, 98, (12,), (4,)), (132, 100, (12,), (2,))])
def test_property_2_integer_cases_are_the_bgr_interpolation_kernel(bbme, shape):
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    CH, CW = H0 // 2, W0 // 2
    c1, c2 = near_colour_pair(w, h, 11 * w + h)
    mf = bbme.MF(c1, c2, list(search), list(block))
    rng = np.random.default_rng(H0)
    for num, den, step in ((1, 2, 2), (1, 3, 3), (2, 3, 3)):
        F, B = (step * rng.integers(-3, 4, (2, CH, CW, 2))).astype(np.int16)
        far = rng.random((CH, CW)) < 0.1
        F[far] *= 40
        for Bk in (B, None):
            exp = _device_bgr(mf, F, Bk, num, 1, den)
            got = _device(mf, (4 * F).astype(np.int16), None if Bk is None else (4 * Bk).astype(np.int16), num, 1, den)
            assert np.array_equal(got, exp), (num, den, Bk is not None)
    mf.close()


def _single(bbme, p):
    """The products of a single context fed pair p of the colour video (computed once)"""
    if p not in _cache:
        video = colour_video(bbme)
        mf = bbme.MF(video[p], video[p + 1], *VIDEO_PARAMS)
        mf.estimate_bidirectional_async()
        _cache[p] = dict(half=mf.interpolate_subpel_bgr(1, 2), run=mf.interpolate_run_subpel_bgr(3))
        if p == 0:
            I1, I2 = mf.get_level_planes(0)
            exp = np_subpel_interpolate_bgr(I1, I2, video[0], video[1], mf.subpel_cells("forward"), mf.subpel_cells("backward"), 1, 2,
                                            mf.padding_x, mf.padding_y)
            assert np.array_equal(_cache[p]["half"], exp)
            assert not np.array_equal(_cache[p]["half"], mf.interpolate_bgr(1, 2))
        mf.close()
    return _cache[p]


def test_batch_and_chain_equal_single_contexts(bbme):
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    singles = [_single(bbme, p) for p in range(4)]
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(2)], search, block)
    chain = bbme.MFChain(video[:3], search, block)
    for ctx, what in ((batch, "batch"), (chain, "chain")):
        ctx.estimate_bidirectional_async()
        for p in (1, 0):
            assert np.array_equal(ctx.get_pair_interpolated_subpel_bgr(p, 1, 2), singles[p]["half"]), (what, p)
            assert np.array_equal(ctx.interpolate_run_subpel_bgr(3, pair=p), singles[p]["run"]), (what, p)
        assert np.array_equal(ctx.interpolate_subpel_bgr(1, 2), singles[0]["half"]), what      # the inherited call addresses pair 0
    batch.close()
    chain.advance(video[3:5], wait=False)                   # pairs (2, 3) and (3, 4)
    chain.estimate_bidirectional_async()
    for p in range(2):
        assert np.array_equal(chain.get_pair_interpolated_subpel_bgr(p, 1, 2), singles[2 + p]["half"]), p
        assert np.array_equal(chain.interpolate_run_subpel_bgr(3, pair=p), singles[2 + p]["run"]), p
    chain.close()


def test_direction_backward_exchanges_the_colour_frames_too(bbme):
    shape = (130, 98, (12,), (4,))
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    c1, c2 = near_colour_pair(w, h, 77)
    I1, I2 = luma_planes(c1, c2, px, py)
    qf, qb = fraction_grids(H0, W0, 5)
    mf = bbme.MF(c1, c2, list(search), list(block))
    swapped = bbme.MF(c2, c1, list(search), list(block))
    mf.set_direction(True)
    for colour in (None, (c1, c2)):                         # stored colour, and a caller's frames in the order they were set
        got = _device(mf, qf, qb, 1, 2, 3, colour, out_extra=1)
        exp = _device(swapped, qf, qb, 1, 2, 3, None if colour is None else (c2, c1), out_extra=1)
        assert np.array_equal(got, exp)
        assert np.array_equal(got[0], np_subpel_interpolate_bgr(I2, I1, c2, c1, qf, qb, 1, 3, px, py))
    mf.set_direction(False)
    mf.close()
    swapped.close()


def test_a_grey_setter_withdraws_the_stored_colour(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    search, block = VIDEO_PARAMS
    c1, c2 = colour_video(bbme)[:2]
    g1, g2 = np_bgr_to_gray(c1), np_bgr_to_gray(c2)
    h, w = g1.shape
    mf = bbme.MF(c1, c2, search, block)
    CH, CW = mf.cells_shape
    z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    out = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    t1, t2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    torch.cuda.synchronize()
    calls = (lambda: mf.interpolate_subpel_bgr(1, 2), lambda: mf.interpolate_run_subpel_bgr(2),
             lambda: mf.cells_interpolate_subpel_bgr_device(z, None, out=out))
    # the two context-level calls need a valid pair of fields; the one that takes grids does not
    assert [_status(bbme, c) for c in calls[:2]] == [_capi.ERR_STATE] * 2
    mf.cells_interpolate_subpel_bgr_device(z, None, out=out)
    mf.estimate_bidirectional_async()
    half = mf.interpolate_subpel_bgr(1, 2)
    grey_half = mf.interpolate_subpel(1, 2)
    mf.set_frames(g1, g2)
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.interpolate_subpel(1, 2), grey_half)                   # the same luma: the grey products stand
    assert [_status(bbme, c) for c in calls] == [_capi.ERR_STATE] * 3
    mf.cells_interpolate_subpel_bgr_device(z, None, t1, t2, out=out)                # a caller's colour needs none stored
    mf.set_frames(c1, c2)
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.interpolate_subpel_bgr(1, 2), half)
    mf.close()


def test_the_calls_change_no_state_and_refuse_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    c1, c2 = colour_video(bbme)[:2]
    h, w = c1.shape[:2]
    mf = bbme.MF(c1, c2, search, block)
    mf.estimate_bidirectional_async()
    CH, CW = mf.cells_shape

    def state():
        return [mf.get_cells(), mf.get_backward_cells(), *mf.get_level_planes(0), mf.interpolate_subpel(1, 2), mf.get_flow()]

    before = state()
    qf, qb = mf.subpel_cells("forward"), mf.subpel_cells("backward")
    tf, tb = _cuda(qf), _cuda(qb)
    t1, t2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    out = torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    half, run = mf.interpolate_subpel_bgr(1, 2), mf.interpolate_run_subpel_bgr(4)
    for colour in ((None, None), (t1, t2)):
        mf.cells_interpolate_subpel_bgr_device(tf, tb, *colour, num0=1, count=3, den=4, out=out)
        mf.synchronize()
        assert np.array_equal(out.cpu().numpy(), run)
    assert all(np.array_equal(a, b) for a, b in zip(before, state()))               # no state changed
    assert np.array_equal(mf.interpolate_subpel_bgr(1, 2), half)
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    f_, b_, o_, p1, p2 = (C.c_void_p(t.data_ptr()) for t in (tf, tb, out, t1, t2))
    buf = np.zeros((h, w, 3), np.uint8)

    def cells(pair=0, f=f_, b=b_, qp=CW, c1=None, c2=None, cp=3 * w, num0=1, count=1, den=2, o=o_, op=3 * w, os=3 * w * h):
        return L.bbme_cells_subpel_interpolate_bgr_device(ctx, pair, f, b, qp, c1, c2, cp, num0, count, den, o, op, os, None)

    def own(pair=0, num0=1, count=1, den=2, o=o_, op=3 * w, os=3 * w * h):
        return L.bbme_subpel_interpolate_bgr_device(ctx, pair, num0, count, den, o, op, os, None)

    assert cells() == 0 and own() == 0 and cells(b=None) == 0 and cells(c1=p1, c2=p2) == 0
    assert cells(count=3, den=4) == 0 and own(count=3, den=4) == 0
    for pair in (-1, 1):
        assert cells(pair=pair) == inv and own(pair=pair) == inv
        assert L.bbme_get_subpel_interpolated_bgr_host(ctx, pair, 1, 2, buf.ctypes.data) == inv
    assert cells(f=None) == inv and cells(o=None) == inv and own(o=None) == inv
    assert L.bbme_get_subpel_interpolated_bgr_host(ctx, 0, 1, 2, None) == inv
    assert cells(qp=CW - 1) == inv                                                  # q4_pitch_cells < CW
    assert cells(c1=p1) == inv and cells(c2=p2) == inv                             # exactly one colour pointer null
    assert cells(c1=p1, c2=p2, cp=3 * w - 1) == inv                                # bgr_pitch < 3 W
    assert cells(cp=0) == 0                                                          # the stored colour has its own pitch
    assert cells(op=3 * w - 1) == inv and own(op=3 * w - 1) == inv                  # out_pitch < 3 W
    assert cells(count=2, den=3, os=3 * w * h - 1) == inv and own(count=2, den=3, os=3 * w * h - 1) == inv    # a stride below one frame
    assert cells(count=1, den=3, os=0) == 0 and own(count=1, den=3, os=0) == 0          # one frame has no stride
    for den in (1, 0, -3, 257):
        assert cells(den=den) == inv and own(den=den) == inv, den
        assert L.bbme_get_subpel_interpolated_bgr_host(ctx, 0, 1, den, buf.ctypes.data) == inv
    for num0, count, den in ((0, 1, 2), (2, 1, 2), (1, 0, 4), (1, 4, 4), (3, 2, 4), (256, 1, 256)):
        assert cells(num0=num0, count=count, den=den) == inv and own(num0=num0, count=count, den=den) == inv, (num0, count, den)
    assert _status(bbme, lambda: mf.interpolate_run_subpel_bgr(1)) == inv
    assert _status(bbme, lambda: mf.cells_interpolate_subpel_bgr_device(tf, tb, t1[:, :w - 1], t2[:, :w - 1], out=out[:1])) == inv
    wide = torch.zeros((CH, CW + 1, 2), dtype=torch.int16, device="cuda")
    assert _status(bbme, lambda: mf.cells_interpolate_subpel_bgr_device(tf, wide[:, :CW], out=out[:1])) == inv
    mf.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(before, state()))
    assert np.array_equal(mf.interpolate_subpel_bgr(1, 2), half)
    mf.close()
    # a context without frames
    ctx = C.c_void_p()
    params = _capi.make_params(search, block)
    assert L.bbme_create(C.byref(params), w, h, 0, C.byref(ctx)) == 0
    assert L.bbme_cells_subpel_interpolate_bgr_device(ctx, 0, f_, None, CW, p1, p2, 3 * w, 1, 1, 2, o_, 3 * w, 0, None) == _capi.ERR_STATE
    assert L.bbme_subpel_interpolate_bgr_device(ctx, 0, 1, 1, 2, o_, 3 * w, 0, None) == _capi.ERR_STATE
    assert L.bbme_get_subpel_interpolated_bgr_host(ctx, 0, 1, 2, buf.ctypes.data) == _capi.ERR_STATE
    assert L.bbme_destroy(ctx) == 0


def _guarded_results(bbme):
    """The colour calls of one single, one batch and one chain context -> sha256 of every result"""
    w, h, search, block = 130, 98, [12], [4]
    grey = bbme.synth_video(w, h, 3, 5, max_motion=3)
    frames = [np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1)) for v in grey]
    results = []
    mf = bbme.MF(frames[0], frames[1], search, block)
    assert (mf.padding_x, mf.padding_y) == (1, 1)
    mf.estimate_bidirectional_async()
    results += [mf.interpolate_subpel_bgr(1, 2), mf.interpolate_run_subpel_bgr(3)]
    qf, qb = fraction_grids(mf.padded_height, mf.padded_width, 1)
    results.append(_device(mf, qf, qb, 1, 2, 3, out_extra=1, q_extra=1))
    results.append(_device(mf, qf, None, 1, 1, 2, (frames[0], frames[1]), colour_extra=1, out_extra=3))
    E, _ = edge_grid(mf.padded_height, mf.padded_width, 1, 2, 13)
    results.append(_device(mf, E, (-E).astype(np.int16), 1, 1, 2))
    ctxs = [mf, bbme.MFBatch([(frames[0], frames[1]), (frames[1], frames[2])], search, block), bbme.MFChain(frames, search, block)]
    for ctx in ctxs[1:]:
        ctx.estimate_bidirectional_async()
        results.append(ctx.get_pair_interpolated_subpel_bgr(1, 1, 3))
    return ctxs, hashlib.sha256(b"".join(np.ascontiguousarray(r).tobytes() for r in results)).hexdigest()


def _guard_child():
    """Runs in a fresh process under BBME_TEST_GUARD=1 and BBME_TEST_POISON=1: prints the digest of the results and the guards' state"""
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    assert os.environ["BBME_TEST_GUARD"] == "1" and os.environ["BBME_TEST_POISON"] == "1"
    ctxs, digest = _guarded_results(bbme)
    live, violations, first = C.c_ulonglong(), C.c_ulonglong(), C.create_string_buffer(512)
    found = C.c_void_p()
    _capi.check(_capi.lib().bbme_test_guard_find(b"the quarter-pel cells of the interpolation", 1, C.byref(found)))
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
    for ctx in ctxs:
        ctx.close()
    after = C.c_ulonglong()
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(after), first, len(first)))
    print("GUARDED %s buffer=%d violations=%d after_close=%d %s" % (digest, bool(found.value), violations.value, after.value,
                                                                     first.value.decode()))


def test_guard_bands_and_poison(bbme):
    """Between guard bands and on poisoned buffers the colour calls damage no band and give the bytes they give without the knobs."""
    ctxs, digest = _guarded_results(bbme)
    for ctx in ctxs:
        ctx.close()
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBME_TEST_GUARD="1", BBME_TEST_POISON="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_subpel_interpolation_bgr as t; t._guard_child()" % (
        tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:5] == [digest, "buffer=1", "violations=0", "after_close=0"], line[0]


@pytest.mark.parametrize("factor", [2, 3])
def test_interpolate_frames_subpel_bgr(bbme, factor):
    from blockbasedmotionestimation_amd.sequence import interpolate_frames
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    got = interpolate_frames(video, search, block, factor, in_flight=4, batch=2, subpel_bgr=True)
    assert len(got) == factor * 4 + 1
    for p in range(4):
        assert np.array_equal(got[factor * p], video[p]), p
        single = _single(bbme, p)
        for k in range(1, factor):
            exp = single["half"] if factor == 2 else single["run"][k - 1]
            assert got[factor * p + k].shape == (VIDEO[1], VIDEO[0], 3)
            assert np.array_equal(got[factor * p + k], exp), (p, k)
    assert np.array_equal(got[-1], video[4])
    if factor == 2:
        with pytest.raises(ValueError):
            interpolate_frames([v[..., 0] for v in video], search, block, factor, subpel_bgr=True)


def test_cli_writes_the_quarter_pel_colour_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    video = colour_video(bbme)
    c1, c2 = (np.ascontiguousarray(v[:72, :96]) for v in video[:2])
    _write_ppm(tmp_path / "f1.ppm", c1)
    _write_ppm(tmp_path / "f2.ppm", c2)
    base = [_build.CLI, str(tmp_path / "f1.ppm"), str(tmp_path / "f2.ppm"), "--levels", "3", "--block", "16", "--search", "30"]
    r = subprocess.run(base + ["--no-upsample", "--interpolate-subpel", str(tmp_path / "mid"), "--factor", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(c1, c2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    px, py, w, h = mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height
    run, grey = mf.interpolate_run_subpel_bgr(3), mf.interpolate_run_subpel(3)
    mf.close()
    for k in (1, 2):
        assert (tmp_path / ("mid_%d.ppm" % k)).read_bytes() == b"P6\n96 72\n255\n" + np.ascontiguousarray(run[k - 1][..., ::-1]).tobytes(), k
        frame = grey[k - 1][py:py + h, px:px + w]
        assert (tmp_path / ("mid_%d.pgm" % k)).read_bytes() == b"P5\n%d %d\n255\n" % (w, h) + frame.tobytes(), k
    assert not (tmp_path / "mid_3.ppm").exists()
