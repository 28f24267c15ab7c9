"""Colour video on the GPU (include/bbme.h, "LUMA RULE" and "BGR INTERPOLATION RULE"), all bit-exact: the *_bgr setters make the
planes, pyramid and cells of the grey setters on the luma (host, async and device forms, pitches above 3 W and 3 W + 1);
k_interpolate_bgr gives the numpy restatement of the rule (test_bgr_cpu.np_interpolate_bgr) on geometries with odd paddings and cut
runs, with injected grids and the context's own fields, caller's and stored colour, output pitches that reach the byte path; grey
frames give the grey result in every channel; batches and chains equal single contexts and the roll carries the colour; direction
BACKWARD equals the exchanged pair; a grey setter withdraws the stored colour; bad arguments are refused and nothing changes
context state; sequence.interpolate_frames and bbme_cli produce the same frames."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _status
from test_bgr_cpu import SHAPES, colour_pair, luma_planes, np_bgr_to_gray, np_interpolate_bgr
from test_interpolation_cpu import random_grids

pytestmark = pytest.mark.gpu

VIDEO = (200, 136, 5, 77, 6)                               # synth_video(width, height, frames, seed, max_motion=...)
VIDEO_PARAMS = ([30, 30, 30], [16, 16, 16])
_cache = {}


def colour_video(bbme):
    """Five colour frames that move like synth_video's grey ones: three different pointwise maps of one video."""
    if "video" not in _cache:
        grey = bbme.synth_video(*VIDEO[:4], max_motion=VIDEO[4])
        _cache["video"] = [np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))
                           for v in grey]
    return _cache["video"]


def _pitched(frame, pitch):
    """The frame's rows `pitch` bytes apart in one buffer, 0xAA between them."""
    h, w = frame.shape[:2]
    buf = np.full(h * pitch, 0xAA, np.uint8)
    for y in range(h):
        buf[y * pitch:y * pitch + 3 * w] = frame[y].reshape(-1)
    return buf


def _grey_reference(bbme, c1, c2):
    """Planes of every level and the cells of a context fed the lumas as grey frames (computed once)."""
    key = ("grey", c1.shape)
    if key not in _cache:
        search, block = VIDEO_PARAMS
        mf = bbme.MF(np_bgr_to_gray(c1), np_bgr_to_gray(c2), search, block)
        planes = [mf.get_level_planes(l) for l in range(3)]
        mf.estimate_async()
        _cache[key] = (planes, mf.get_cells())
        mf.close()
    return _cache[key]


@pytest.mark.parametrize("kind", ["host", "host_async", "device"])
@pytest.mark.parametrize("extra", [5, 1])
def test_bgr_setters_make_the_grey_setters_planes(bbme, kind, extra):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    c1, c2 = colour_video(bbme)[:2]
    h, w = c1.shape[:2]
    planes, cells = _grey_reference(bbme, c1, c2)
    px, py = bbme.plan_padding(w, h, search, block)[2:]
    assert np.array_equal(planes[0][0], np.pad(np_bgr_to_gray(c1), ((py, py), (px, px))))
    mf = bbme.MF(np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), search, block)
    pitch = 3 * w + extra
    b1, b2 = _pitched(c1, pitch), _pitched(c2, pitch)
    if kind == "device":
        t1, t2 = torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda()
        torch.cuda.synchronize()
        _capi.check(L.bbme_set_frames_device_bgr(mf._ctx, 0, C.c_void_p(t1.data_ptr()), C.c_void_p(t2.data_ptr()), pitch))
    elif kind == "host_async":
        _capi.check(L.bbme_set_frames_host_bgr_async(mf._ctx, 0, b1.ctypes.data, b2.ctypes.data, pitch))
        mf.synchronize()
    else:
        _capi.check(L.bbme_set_frames_host_bgr(mf._ctx, 0, b1.ctypes.data, b2.ctypes.data, pitch))
    for level in range(3):
        got = mf.get_level_planes(level)
        assert np.array_equal(got[0], planes[level][0]) and np.array_equal(got[1], planes[level][1]), level
    mf.estimate_async()
    assert np.array_equal(mf.get_cells(), cells)
    # the store holds the frames themselves: the stored colour and the caller's give one result
    mf.estimate_bidirectional_async()
    stored = mf.interpolate_bgr(1, 2)
    I1, I2 = planes[0]
    assert np.array_equal(stored, np_interpolate_bgr(I1, I2, c1, c2, mf.get_cells(), mf.get_backward_cells(), 1, 2, px, py))
    mf.close()


@pytest.mark.parametrize("kind", ["host", "host_async", "device"])
def test_chain_bgr_setters_take_a_pitch_of_3w_plus_1(bbme, kind):
    """The run forms (k_bgr_pad_run, the pitched upload into the store) through the C-ABI: slots 1 and 2 of a chain from
    frames whose rows are 3 W + 1 bytes apart, after slot 0 from packed rows."""
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)[:3]
    h, w = video[0].shape[:2]
    grey = bbme.MFChain([np_bgr_to_gray(v) for v in video], search, block)
    chain = bbme.MFChain([np.zeros((h, w), np.uint8)] * 3, search, block, frames_on_device=False)
    chain.set_frame_run(0, [video[0]])
    pitch = 3 * w + 1
    bufs = [_pitched(v, pitch) for v in video[1:]]
    if kind == "device":
        tensors = [torch.from_numpy(b).cuda() for b in bufs]
        torch.cuda.synchronize()
        table = (C.c_void_p * 2)(*[t.data_ptr() for t in tensors])
        _capi.check(L.bbme_set_chain_frames_device_bgr(chain._ctx, 1, 2, table, pitch))
    else:
        table = (C.c_void_p * 2)(*[b.ctypes.data for b in bufs])
        setter = L.bbme_set_chain_frames_host_bgr if kind == "host" else L.bbme_set_chain_frames_host_bgr_async
        _capi.check(setter(chain._ctx, 1, 2, table, pitch))
    chain.synchronize()
    for level in range(3):
        for slot in range(3):
            assert np.array_equal(chain.get_slot_plane(level, slot), grey.get_slot_plane(level, slot)), (level, slot)
    grey.close()
    chain.estimate_bidirectional_async()
    for p in range(2):
        single = _single(bbme, p)
        assert np.array_equal(chain.get_pair_cells(p), single["cells"]), p
        assert np.array_equal(chain.interpolate_bgr(1, 2, pair=p), single["half"]), p          # the stored colour is the frames'
    chain.close()


def _device_bgr(mf, f, b, num0, count, den, colour=None, colour_extra=0, out_extra=0, stream=None, pair=0):
    """cells_interpolate_bgr_device on host grids -> (count, H, W, 3) numpy; colour = (c1, c2) host frames handed over as tensors
    whose rows are colour_extra bytes further apart than packed, None = the stored colour; the output's rows out_extra bytes
    further apart than packed, and those bytes stay untouched."""
    import torch
    h, w = mf.orig_height, mf.orig_width
    tf = torch.from_numpy(np.ascontiguousarray(f)).cuda()
    tb = None if b is None else torch.from_numpy(np.ascontiguousarray(b)).cuda()
    t1 = t2 = None
    if colour is not None:
        t1, t2 = (torch.from_numpy(_pitched(c, 3 * w + colour_extra)).cuda().as_strided((h, w, 3), (3 * w + colour_extra, 3, 1))
                  for c in colour)
    pitch = 3 * w + out_extra
    raw = torch.full((count * h * pitch + 3,), 0xAA, dtype=torch.uint8, device="cuda")
    out = raw.as_strided((count, h, w, 3), (h * pitch, pitch, 3, 1))
    torch.cuda.synchronize()
    mf.cells_interpolate_bgr_device(tf, tb, t1, t2, num0, count, den, pair=pair, out=out,
                                    hip_stream_handle=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    rows = raw[:count * h * pitch].view(count * h, pitch)
    assert bool((rows[:, 3 * w:] == 0xAA).all()) and bool((raw[count * h * pitch:] == 0xAA).all())
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_interpolate_bgr_equals_numpy(bbme, shape):
    import torch
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    c1, c2 = colour_pair(w, h, 7 * w + h)
    mf = bbme.MF(c1, c2, list(search), list(block))
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == SHAPES[shape]
    I1, I2 = mf.get_level_planes(0)
    e1, e2 = luma_planes(c1, c2, px, py)
    assert np.array_equal(I1, e1) and np.array_equal(I2, e2)
    rng = np.random.default_rng(w + h)
    f, b = random_grids(H0 // 2, W0 // 2, rng)
    # (num0, count, den, backward grid, caller's colour, its extra pitch, the output's extra pitch)
    for num0, count, den, with_b, own, c_extra, o_extra in ((1, 1, 2, True, False, 0, 0), (1, 3, 4, True, True, 0, 1),
                                                            (1, 1, 3, False, True, 1, 3), (2, 3, 5, False, False, 0, 3),
                                                            (255, 1, 256, True, True, 7, 0), (1, 3, 4, True, False, 0, 0)):
        got = _device_bgr(mf, f, b if with_b else None, num0, count, den, (c1, c2) if own else None, c_extra, o_extra)
        for q in range(count):
            exp = np_interpolate_bgr(I1, I2, c1, c2, f, b if with_b else None, num0 + q, den, px, py)
            assert np.array_equal(got[q], exp), (num0 + q, den, with_b, own, c_extra, o_extra)
    got = _device_bgr(mf, f, b, 1, 2, 3, stream=torch.cuda.Stream())
    assert np.array_equal(got[1], np_interpolate_bgr(I1, I2, c1, c2, f, b, 2, 3, px, py))
    # the context's own fields
    mf.estimate_bidirectional_async()
    fwd, bwd = mf.get_cells(), mf.get_backward_cells()
    assert np.array_equal(mf.interpolate_bgr(1, 2), np_interpolate_bgr(I1, I2, c1, c2, fwd, bwd, 1, 2, px, py))
    run = mf.interpolate_run_bgr(4)
    assert run.shape == (3, h, w, 3)
    for num in (1, 2, 3):
        assert np.array_equal(run[num - 1], np_interpolate_bgr(I1, I2, c1, c2, fwd, bwd, num, 4, px, py)), num
    mf.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gray_frames_give_the_grey_frame_in_every_channel(bbme, shape):
    w, h, search, block = shape
    _, _, px, py = SHAPES[shape]
    g1, g2, _ = bbme.synth_pair(w, h, 300 + w + h, max_motion=3)
    mf = bbme.MF(np.repeat(g1[..., None], 3, 2), np.repeat(g2[..., None], 3, 2), list(search), list(block))
    mf.estimate_bidirectional_async()
    for num, den in ((1, 2), (2, 3)):
        grey = mf.interpolate(num, den)[py:py + h, px:px + w]
        got = mf.interpolate_bgr(num, den)
        for ch in range(3):
            assert np.array_equal(got[..., ch], grey), (num, den, ch)
    ref = bbme.MF(g1, g2, list(search), list(block))
    ref.estimate_bidirectional_async()
    assert np.array_equal(ref.interpolate(1, 2), mf.interpolate(1, 2))
    ref.close()
    mf.close()


def _single(bbme, p):
    """The colour products of a single context fed pair p = (frame p, frame p + 1) of the colour video (computed once)."""
    key = ("single", p)
    if key not in _cache:
        video = colour_video(bbme)
        mf = bbme.MF(video[p], video[p + 1], *VIDEO_PARAMS)
        mf.estimate_bidirectional_async()
        _cache[key] = dict(half=mf.interpolate_bgr(1, 2), run=mf.interpolate_run_bgr(3), cells=mf.get_cells(),
                           back=mf.get_backward_cells(), grey=mf.interpolate(1, 2))
        mf.close()
    return _cache[key]


def test_batch_and_chain_equal_single_contexts(bbme):
    import torch
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    singles = [_single(bbme, p) for p in range(4)]
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(2)], search, block)
    chain = bbme.MFChain(video[:3], search, block)
    for ctx, what in ((batch, "batch"), (chain, "chain")):
        ctx.estimate_bidirectional_async()
        for p in range(2):
            assert np.array_equal(ctx.get_pair_cells(p), singles[p]["cells"]), (what, p)
            assert np.array_equal(ctx.interpolate_bgr(1, 2, pair=p), singles[p]["half"]), (what, p)
            assert np.array_equal(ctx.interpolate_run_bgr(3, pair=p), singles[p]["run"]), (what, p)
            assert np.array_equal(ctx.get_pair_interpolated(p), singles[p]["grey"]), (what, p)
    batch.close()
    # the roll carries the last slot's colour to slot 0: pairs (2, 3) and (3, 4)
    chain.advance(video[3:5], wait=False)
    chain.estimate_bidirectional_async()
    for p in range(2):
        assert np.array_equal(chain.interpolate_bgr(1, 2, pair=p), singles[2 + p]["half"]), p
        assert np.array_equal(chain.interpolate_run_bgr(3, pair=p), singles[2 + p]["run"]), p
    chain.close()
    # frames in HBM: a chain and a batch fed torch tensors
    tv = [torch.from_numpy(v).cuda() for v in video[:3]]
    torch.cuda.synchronize()
    chain = bbme.MFChain(tv, search, block, frames_on_device=True)
    batch = bbme.MFBatch([(tv[0], tv[1]), (tv[1], tv[2])], search, block, frames_on_device=True)
    for ctx in (chain, batch):
        ctx.estimate_bidirectional_async()
        for p in range(2):
            assert np.array_equal(ctx.interpolate_bgr(1, 2, pair=p), singles[p]["half"]), p
        ctx.close()


def test_direction_backward_exchanges_the_colour_frames_too(bbme):
    shape = (130, 98, (12,), (4,))
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    c1, c2 = colour_pair(w, h, 77)
    I1, I2 = luma_planes(c1, c2, px, py)
    f, b = random_grids(H0 // 2, W0 // 2, np.random.default_rng(5))
    mf = bbme.MF(c1, c2, list(search), list(block))
    swapped = bbme.MF(c2, c1, list(search), list(block))
    mf.set_direction(True)
    for colour in (None, (c1, c2)):                         # stored colour, and a caller's frames in the order they were set
        got = _device_bgr(mf, f, b, 1, 2, 3, colour, out_extra=1)
        exp = _device_bgr(swapped, f, b, 1, 2, 3, None if colour is None else (c2, c1), out_extra=1)
        assert np.array_equal(got, exp)
        assert np.array_equal(got[0], np_interpolate_bgr(I2, I1, c2, c1, f, b, 1, 3, px, py))
    mf.estimate_bidirectional_async()                      # leaves the direction forward
    swapped.estimate_bidirectional_async()
    swapped.set_direction(True)
    swapped.estimate_bidirectional_async()
    assert np.array_equal(mf.interpolate_bgr(1, 2), np_interpolate_bgr(I1, I2, c1, c2, mf.get_cells(), mf.get_backward_cells(), 1, 2, px, py))
    mf.close()
    swapped.close()


def test_a_grey_setter_withdraws_the_stored_colour(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    c1, c2 = video[:2]
    g1, g2 = np_bgr_to_gray(c1), np_bgr_to_gray(c2)
    h, w = g1.shape
    mf = bbme.MF(c1, c2, search, block)
    CH, CW = mf.cells_shape
    z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    out = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    t1, t2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    torch.cuda.synchronize()
    colour_calls = (lambda: mf.interpolate_bgr(1, 2), lambda: mf.interpolate_run_bgr(2),
                    lambda: mf.cells_interpolate_bgr_device(z, None, out=out), lambda: mf.bgr_frames_device_ptrs())
    # the two context-level calls need a valid pair of fields; the one that takes grids, and the pointers, do not
    assert [_status(bbme, c) for c in colour_calls[:2]] == [_capi.ERR_STATE] * 2
    mf.cells_interpolate_bgr_device(z, None, out=out)
    assert all(mf.bgr_frames_device_ptrs())
    mf.estimate_bidirectional_async()
    half = mf.interpolate_bgr(1, 2)
    grey_half = mf.interpolate(1, 2)
    for grey_setter in (lambda: mf.set_frames(g1, g2), lambda: mf.set_frames_device(torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()),
                        lambda: mf.set_level_planes(0, *mf.get_level_planes(0))):
        grey_setter()
        mf.estimate_bidirectional_async()
        assert np.array_equal(mf.interpolate(1, 2), grey_half)                    # the same luma: the grey products stand
        assert [_status(bbme, c) for c in colour_calls] == [_capi.ERR_STATE] * 4
        mf.cells_interpolate_bgr_device(z, None, t1, t2, out=out)                    # a caller's colour needs none stored
        mf.set_frames(c1, c2)
        mf.estimate_bidirectional_async()
        assert np.array_equal(mf.interpolate_bgr(1, 2), half)
    mf.close()
    # a chain: a grey setter of ONE slot withdraws the colour of the two pairs that read it, and of no other
    chain = bbme.MFChain(video[:4], search, block)
    chain.estimate_bidirectional_async()
    halves = [chain.interpolate_bgr(1, 2, pair=p) for p in range(3)]
    chain.set_frame_run(1, [np_bgr_to_gray(video[1])])
    chain.estimate_bidirectional_async()
    assert _status(bbme, lambda: chain.interpolate_bgr(1, 2, pair=0)) == _capi.ERR_STATE
    assert _status(bbme, lambda: chain.interpolate_bgr(1, 2, pair=1)) == _capi.ERR_STATE
    assert np.array_equal(chain.interpolate_bgr(1, 2, pair=2), halves[2])
    chain.set_frame_run(1, [video[1]])
    chain.estimate_bidirectional_async()
    for p in range(3):
        assert np.array_equal(chain.interpolate_bgr(1, 2, pair=p), halves[p]), p
    # the roll of a grey last slot leaves slot 0 without colour
    chain.set_frame_run(3, [np_bgr_to_gray(video[3])])
    chain.advance([video[4]] * 3)
    chain.estimate_bidirectional_async()
    assert _status(bbme, lambda: chain.interpolate_bgr(1, 2, pair=0)) == _capi.ERR_STATE
    chain.interpolate_bgr(1, 2, pair=1)
    chain.close()


def test_colour_calls_change_no_state_and_refuse_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = VIDEO_PARAMS
    c1, c2 = colour_video(bbme)[:2]
    h, w = c1.shape[:2]
    mf = bbme.MF(c1, c2, search, block)
    mf.estimate_bidirectional_async()

    def state():
        return dict(flow=mf.get_flow(), cells=mf.get_cells(), back=mf.get_backward_cells(), grey=mf.interpolate(1, 2),
                    stats=mf.interpolation_stats(1, 2))

    before = state()
    tf, tb = torch.from_numpy(before["cells"]).cuda(), torch.from_numpy(before["back"]).cuda()
    t1, t2 = torch.from_numpy(c1).cuda(), torch.from_numpy(c2).cuda()
    out = torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    half = mf.interpolate_bgr(1, 2)
    mf.cells_interpolate_bgr_device(tf, tb, num0=1, count=3, den=4, out=out)
    mf.synchronize()
    assert np.array_equal(out.cpu().numpy(), mf.interpolate_run_bgr(4))
    mf.cells_interpolate_bgr_device(tf, tb, t1, t2, num0=1, count=3, den=4, out=out)
    mf.synchronize()
    assert np.array_equal(out.cpu().numpy(), mf.interpolate_run_bgr(4))
    after = state()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    f_, b_, o_, p1, p2 = (C.c_void_p(t.data_ptr()) for t in (tf, tb, out, t1, t2))
    buf = np.zeros((h, w, 3), np.uint8)

    def cells(pair=0, f=f_, b=b_, c1=None, c2=None, cp=3 * w, num0=1, count=1, den=2, o=o_, op=3 * w, os=3 * w * h):
        return L.bbme_cells_interpolate_bgr_device(ctx, pair, f, b, c1, c2, cp, num0, count, den, o, op, os, None)

    def own(pair=0, num0=1, count=1, den=2, o=o_, op=3 * w, os=3 * w * h):
        return L.bbme_interpolate_bgr_device(ctx, pair, num0, count, den, o, op, os, None)

    assert cells() == 0 and own() == 0 and cells(b=None) == 0 and cells(c1=p1, c2=p2) == 0
    assert cells(count=3, den=4) == 0 and own(count=3, den=4) == 0
    for pair in (-1, 1):
        assert cells(pair=pair) == inv and own(pair=pair) == inv
        assert L.bbme_get_interpolated_bgr_host(ctx, pair, 1, 2, buf.ctypes.data) == inv
    assert cells(f=None) == inv and cells(o=None) == inv and own(o=None) == inv
    assert L.bbme_get_interpolated_bgr_host(ctx, 0, 1, 2, None) == inv
    assert cells(c1=p1) == inv and cells(c2=p2) == inv                             # one colour frame without the other
    assert cells(c1=p1, c2=p2, cp=3 * w - 1) == inv
    assert cells(cp=0) == 0                                                          # the stored colour has its own pitch
    assert cells(op=3 * w - 1) == inv and own(op=3 * w - 1) == inv
    assert cells(count=2, den=3, os=3 * w * h - 1) == inv and own(count=2, den=3, os=3 * w * h - 1) == inv
    assert cells(count=1, den=3, os=0) == 0 and own(count=1, den=3, os=0) == 0          # one frame has no stride
    for den in (1, 0, -3, 257):
        assert cells(den=den) == inv and own(den=den) == inv, den
        assert L.bbme_get_interpolated_bgr_host(ctx, 0, 1, den, buf.ctypes.data) == inv
    for num0, count, den in ((0, 1, 2), (2, 1, 2), (1, 0, 4), (1, 4, 4), (3, 2, 4), (256, 1, 256)):
        assert cells(num0=num0, count=count, den=den) == inv and own(num0=num0, count=count, den=den) == inv, (num0, count, den)
    # the setters
    d1, d2 = c1.ctypes.data, c2.ctypes.data
    table = (C.c_void_p * 2)(d1, d2)
    for setter in (L.bbme_set_frames_host_bgr, L.bbme_set_frames_host_bgr_async):
        assert setter(ctx, 0, d1, d2, 3 * w - 1) == inv and setter(ctx, 1, d1, d2, 3 * w) == inv and setter(ctx, -1, d1, d2, 3 * w) == inv
        assert setter(ctx, 0, None, d2, 3 * w) == inv and setter(ctx, 0, d1, None, 3 * w) == inv
    assert L.bbme_set_frames_device_bgr(ctx, 0, p1, p2, 3 * w - 1) == inv and L.bbme_set_frames_device_bgr(ctx, 0, p1, None, 3 * w) == inv
    assert L.bbme_set_chain_frames_host_bgr(ctx, 0, 2, table, 3 * w) == _capi.ERR_UNSUPPORTED
    assert L.bbme_bgr_frames_device_pair(ctx, 0, None, None) == inv
    mf.synchronize()
    after = state()                                        # the refused setters touched nothing
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    assert np.array_equal(mf.interpolate_bgr(1, 2), half)
    assert _status(bbme, lambda: mf.interpolate_run_bgr(1)) == inv
    assert _status(bbme, lambda: mf.cells_interpolate_bgr_device(tf, tb, t1[:, :w - 1], t2[:, :w - 1], out=out[:1])) == inv
    mf.close()
    chain = bbme.MFChain(colour_video(bbme)[:3], search, block)
    cc = chain._ctx
    table3 = (C.c_void_p * 3)(d1, d2, d1)
    assert L.bbme_set_frames_host_bgr(cc, 0, d1, d2, 3 * w) == _capi.ERR_UNSUPPORTED
    for setter in (L.bbme_set_chain_frames_host_bgr, L.bbme_set_chain_frames_host_bgr_async, L.bbme_set_chain_frames_device_bgr):
        assert setter(cc, 0, 2, table3, 3 * w - 1) == inv and setter(cc, 2, 2, table3, 3 * w) == inv and setter(cc, -1, 1, table3, 3 * w) == inv
        assert setter(cc, 0, 0, table3, 3 * w) == inv and setter(cc, 0, 2, None, 3 * w) == inv
        assert setter(cc, 0, 2, (C.c_void_p * 2)(d1, None), 3 * w) == inv
    chain.estimate_bidirectional_async()                   # the refused setters left every slot set and coloured
    chain.interpolate_bgr(1, 2, pair=1)
    assert _status(bbme, lambda: bbme.MF(c1, c2, search, block, upsample=4)) == inv      # there is no up-sampled colour
    chain.close()


@pytest.mark.parametrize("factor", [2, 3])
def test_interpolate_frames_in_colour(bbme, factor):
    from blockbasedmotionestimation_amd.sequence import interpolate_frames
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    got = interpolate_frames(video, search, block, factor, in_flight=4, batch=2)
    assert len(got) == factor * 4 + 1
    for p in range(4):
        assert np.array_equal(got[factor * p], video[p]), p
        single = _single(bbme, p)
        for k in range(1, factor):
            exp = single["half"] if factor == 2 else single["run"][k - 1]
            assert got[factor * p + k].shape == (VIDEO[1], VIDEO[0], 3)
            assert np.array_equal(got[factor * p + k], exp), (p, k)
    assert np.array_equal(got[-1], video[4])


def _write_ppm(path, bgr):
    h, w = bgr.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(bgr[..., ::-1]).tobytes())


def test_cli_takes_ppm_frames_and_writes_colour_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    video = colour_video(bbme)
    c1, c2 = (np.ascontiguousarray(v[:72, :96]) for v in video[:2])
    _write_ppm(tmp_path / "f1.ppm", c1)
    _write_ppm(tmp_path / "f2.ppm", c2)
    base = [_build.CLI, str(tmp_path / "f1.ppm"), str(tmp_path / "f2.ppm"), "--levels", "3", "--block", "16", "--search", "30"]
    r = subprocess.run(base + ["--no-upsample", "--interpolate", str(tmp_path / "mid"), "--factor", "3", "--out", str(tmp_path / "c.flo")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(c1, c2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    for k in (1, 2):
        frame = mf.interpolate_bgr(k, 3)
        assert (tmp_path / ("mid_%d.ppm" % k)).read_bytes() == b"P6\n96 72\n255\n" + np.ascontiguousarray(frame[..., ::-1]).tobytes(), k
    assert not (tmp_path / "mid_1.pgm").exists() and not (tmp_path / "mid_3.ppm").exists()
    fl = bbme.Flow()
    fl.WriteFlowFile(mf.get_subsampled_flow(1), str(tmp_path / "d.flo"))
    assert (tmp_path / "c.flo").read_bytes() == (tmp_path / "d.flo").read_bytes()
    mf.close()
    # with the x4 up-sampling the field is the grey pipeline's on the luma; colour frames in between need --no-upsample
    r = subprocess.run(base + ["--out", str(tmp_path / "u.flo")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(np_bgr_to_gray(c1), np_bgr_to_gray(c2), [30] * 3, [16] * 3, upsample=4)
    fl.WriteFlowFile(mf.calcMotionBlockMatchingSubsampled(), str(tmp_path / "v.flo"))
    assert (tmp_path / "u.flo").read_bytes() == (tmp_path / "v.flo").read_bytes()
    mf.close()
    r = subprocess.run(base + ["--interpolate", str(tmp_path / "bad")], capture_output=True, text=True)
    assert r.returncode == 2 and "--no-upsample" in r.stderr
