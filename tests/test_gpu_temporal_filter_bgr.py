"""Temporal filtering of colour frames on the GPU (include/bbme.h, "BGR TEMPORAL FILTER RULE"), all bit-exact: k_temporal_filter_bgr
gives the numpy restatement of the rule (test_temporal_filter_bgr_cpu.np_temporal_filter_bgr) on geometries with odd paddings and
cut runs, on the stored colour with the context's own fields and on a caller's frames and grids (random, int16 extremes; both
neighbours and each alone), with windows, colour and output pitches that reach the byte paths, guard bytes and a side stream; both
divisions are exact in every channel; B = G = R gives the grey filter of the same context; chains filter every slot from both
sides, batches from one; the calls need fields and stored colour, change no context state and refuse bad arguments;
sequence.denoise_frames and bbme_cli produce the same colour frames."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _cuda, _embed, _stats_of, _status
from test_bgr_cpu import SHAPES, np_bgr_to_gray
from test_gpu_bgr import VIDEO, VIDEO_PARAMS, _write_ppm, colour_video
from test_interpolation_cpu import extreme_grids, odd_windows, random_grids
from test_temporal_filter_bgr_cpu import RULE_THRS, in_channel, near_colour_triple, near_grids, np_temporal_filter_bgr
from test_temporal_filter_cpu import (S23_THR, STAT_KEYS, THRS, neighbour_sets, s23_table_planes, s_table_check, s_table_planes,
                                      thr_table_expected, thr_table_planes)

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

_cache = {}


def _pitched_tensor(frame, extra):
    """The (H, W, 3) frame as a CUDA tensor whose rows are 3 W + extra bytes apart, 0xAA between them."""
    import torch
    if frame is None:
        return None
    h, w = frame.shape[:2]
    buf = torch.full((h, 3 * w + extra), 0xAA, dtype=torch.uint8, device="cuda")
    view = buf.as_strided((h, w, 3), (3 * w + extra, 3, 1))
    view.copy_(torch.from_numpy(np.ascontiguousarray(frame)).cuda())
    return view


def _device_filter(mf, Cur, P, GP, N, GN, thr, window=None, colour_extra=0, out_extra=0, stream=None, want=("out", "map", "stats")):
    """cells_temporal_filter_bgr_device on host frames and grids -> (frame (H, W, 3), map (CH, CW), stats tuple), None where not
    asked for.  The colour frames' rows are colour_extra bytes further apart than packed, the rows of both outputs out_extra; the
    bytes between the output's rows and the 64 behind its last row stay 0xAA."""
    import torch
    CH, CW = mf.cells_shape
    h, w = mf.orig_height, mf.orig_width
    tc, tp, tn = (_pitched_tensor(a, colour_extra) for a in (Cur, P, N))
    tgp, tgn = _cuda(GP), _cuda(GN)
    pitch = 3 * w + out_extra
    raw = torch.full((h * pitch + 64,), 0xAA, dtype=torch.uint8, device="cuda") if "out" in want else None
    out = None if raw is None else raw.as_strided((h, w, 3), (pitch, 3, 1))
    wmap = torch.full((CH, CW + out_extra), 0xAA, dtype=torch.uint8, device="cuda") if "map" in want else None
    st = torch.zeros(4, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    mf.cells_temporal_filter_bgr_device(tc, tp, tn, tgp, tgn, thr, out=out, weights=None if wmap is None else wmap[:, :CW], stats=st,
                                        window=window, hip_stream_handle=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    if raw is not None:                                    # the guard bytes between the rows and behind the frame stay untouched
        rows = raw[:h * pitch].view(h, pitch)
        assert bool((rows[:, 3 * w:] == 0xAA).all()) and bool((raw[h * pitch - out_extra:] == 0xAA).all())
    if wmap is not None and out_extra:
        assert bool((wmap[:, CW:] == 0xAA).all())
    return (None if out is None else out.cpu().numpy(), None if wmap is None else wmap[:, :CW].cpu().numpy(),
            None if st is None else tuple(st.cpu().tolist()))


def _assert_device_equals_numpy(mf, Cur, P, GP, N, GN, thr, window=None, what=None, **kw):
    out, wmap, st = _device_filter(mf, Cur, P, GP, N, GN, thr, window, **kw)
    exp = np_temporal_filter_bgr(Cur, P, GP, N, GN, thr, mf.padding_x, mf.padding_y, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert out is None or np.array_equal(out, exp[0]), tag
    assert wmap is None or np.array_equal(wmap, exp[1]), tag
    assert st is None or st == exp[2], tag
    return exp


@pytest.mark.parametrize("shape", list(SHAPES))
def test_temporal_filter_bgr_equals_numpy(bbme, shape):
    import torch
    w, h, search, block = shape
    W0, H0, px, py = SHAPES[shape]
    Cur, P, N = near_colour_triple(w, h, 7 * w + h)
    mf = bbme.MF(Cur, N, list(search), list(block))
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == (W0, H0, px, py)
    CH, CW = mf.cells_shape
    wins = odd_windows(CH, CW)
    # the stored colour with the context's own fields: image 1 with its next neighbour, image 2 with its previous one
    mf.estimate_bidirectional_async()
    fwd, bwd = mf.get_cells(), mf.get_backward_cells()
    own = [(Cur, None, None, N, fwd), (N, Cur, bwd, None, None)]
    for thr in RULE_THRS:
        for which in (0, 1):
            assert np.array_equal(mf.temporal_filter_bgr(thr, which), np_temporal_filter_bgr(*own[which], thr, px, py)[0]), (thr, which)
        for win, np_win in ((None, mf.default_cell_window()), ("all", None), (wins[1], wins[1]), (wins[3], wins[3])):
            got = mf.temporal_filter_bgr_stats(thr, win)
            assert [_stats(g) for g in got] == [np_temporal_filter_bgr(*own[k], thr, px, py, np_win)[2] for k in (0, 1)], (thr, win)
    # a caller's frames and grids: neighbour sets, strengths, windows, colour pitches 3 W + 1 and 3 W + 5, output rows 0, 1 and 3
    # bytes further apart than packed
    rng = np.random.default_rng(3 * w + h)
    gp, gn = near_grids(CH, CW, rng)
    seen = set()
    for n, thr in enumerate(RULE_THRS):
        for k, (p, a, q, b) in enumerate(neighbour_sets(P, gp, N, gn)):
            exp = _assert_device_equals_numpy(mf, Cur, p, a, q, b, thr, wins[(n + k) % len(wins)], shape,
                                              colour_extra=(0, 1, 5)[(n + k) % 3], out_extra=(0, 1, 3)[(n + 2 * k) % 3])
            seen |= set(np.unique(exp[1] & 0x0f).tolist()) | set(np.unique(exp[1] >> 4).tolist())
    assert seen == set(range(9))
    fp, fn = random_grids(CH, CW, rng)                     # vectors that leave the view on every side
    _assert_device_equals_numpy(mf, Cur, P, fp, N, fn, 255, wins[1], "far grids, side stream", colour_extra=1, out_extra=1,
                                stream=torch.cuda.Stream())
    _assert_device_equals_numpy(mf, Cur, P, fp, N, fn, 64, what="frame only", want=("out",), out_extra=3)
    _assert_device_equals_numpy(mf, Cur, P, fp, N, fn, 1021, what="map only", want=("map",), colour_extra=5)
    _assert_device_equals_numpy(mf, Cur, P, fp, N, fn, 64, wins[3], "statistics only", want=("stats",))
    ep, en = extreme_grids(CH, CW, rng)
    for thr in (1, 1021):
        out, wmap, st = _assert_device_equals_numpy(mf, Cur, P, ep, N, en, thr, what="int16 extremes", colour_extra=1)
        assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)
    # the injected frames and grids left the context's own alone
    assert np.array_equal(mf.temporal_filter_bgr(64), np_temporal_filter_bgr(*own[0], 64, px, py)[0])
    mf.close()


@pytest.fixture(scope="module")
def table_context(bbme):
    """A one-level 132 x 100 context without padding: the division tables are injected as tensors."""
    z = np.zeros((100, 132, 3), np.uint8)
    mf = bbme.MF(z, z, [12], [2])
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == (132, 100, 0, 0)
    yield mf
    mf.close()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_divisions_are_exact_in_every_channel_in_the_kernel(table_context, k):
    mf = table_context
    H0, W0 = mf.padded_height, mf.padded_width
    CH, CW = mf.cells_shape
    Cur, N, cost = thr_table_planes()                      # 92 x 92 inside the 132 x 100 frame; the rest is equal: weight 8
    rest = (np.arange(H0 * W0).reshape(H0, W0) * 7 % 251).astype(np.uint8)
    fC, fN = in_channel(_embed(Cur, H0, W0), k, rest), in_channel(_embed(N, H0, W0), k, rest)
    z = np.zeros((CH, CW, 2), np.int16)
    for thr in THRS:
        exp = np.full((CH, CW), 8, np.int64)
        exp[:cost.shape[0], :cost.shape[1]] = thr_table_expected(cost, thr)
        _, wmap, _ = _device_filter(mf, fC, None, None, fN, z, thr, want=("map",))
        assert np.array_equal(wmap >> 4, exp) and not (wmap & 0x0f).any(), thr
        _, wmap, _ = _device_filter(mf, fC, fN, z, None, None, thr, want=("map",))
        assert np.array_equal(wmap, exp), thr
    for planes, thr, pairs, ends in ((s_table_planes(), 64, None, True), (s23_table_planes(), S23_THR, [(8, 7)], False)):
        Cur, P, N, expect_w = planes                       # 132 x 100, the context's own size
        rest = (np.arange(Cur.size).reshape(Cur.shape) * 5 % 256).astype(np.uint8)
        out, wmap, _ = _device_filter(mf, in_channel(Cur, k, rest), in_channel(P, k, rest), z, in_channel(N, k, rest), z, thr)
        s_table_check(Cur, P, N, expect_w, out[..., k], wmap, pairs=pairs, ends=ends)
        for o in range(3):
            if o != k:
                assert np.array_equal(out[..., o], rest)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gray_frames_give_the_grey_filter_of_the_same_context(bbme, shape):
    w, h, search, block = shape
    _, _, px, py = SHAPES[shape]
    g1, g2, _ = bbme.synth_pair(w, h, 300 + w + h, max_motion=3)
    mf = bbme.MF(np.repeat(g1[..., None], 3, 2), np.repeat(g2[..., None], 3, 2), list(search), list(block))
    mf.estimate_bidirectional_async()
    CH, CW = mf.cells_shape
    changed = 0
    for thr in RULE_THRS:
        for which in (0, 1):
            grey = mf.temporal_filter(thr, which)[py:py + h, px:px + w]
            col = mf.temporal_filter_bgr(thr, which)
            for k in range(3):
                assert np.array_equal(col[..., k], grey), (thr, which, k)
            changed += int((grey != (g1, g2)[which]).sum())
        for win in (None, "all", odd_windows(CH, CW)[1]):
            grey = [_stats(s) for s in mf.temporal_filter_stats(thr, win)]
            assert [_stats(s) for s in mf.temporal_filter_bgr_stats(thr, win)] == [(a, b, c, 3 * d) for a, b, c, d in grey], (thr, win)
    assert changed > 0
    mf.close()


def _video_fields(bbme, key, video):
    """Forward and backward cells of every consecutive pair of the colour video, from single contexts (computed once)."""
    if key not in _cache:
        search, block = VIDEO_PARAMS
        fwd, bwd = [], []
        for p in range(len(video) - 1):
            mf = bbme.MF(video[p], video[p + 1], search, block)
            mf.estimate_bidirectional_async()
            fwd.append(mf.get_cells())
            bwd.append(mf.get_backward_cells())
            pads = (mf.padding_x, mf.padding_y)
            mf.close()
        _cache[key] = (fwd, bwd, pads)
    return _cache[key]


def _video_rule(video, fields, f, thr, window=None, side=None):
    """The rule on frame f of the video with the single contexts' fields: both neighbours where they exist, or one `side`."""
    fwd, bwd, (px, py) = fields
    last = len(video) - 1
    prev = f > 0 and side in (None, "prev")
    nxt = f < last and side in (None, "next")
    return np_temporal_filter_bgr(video[f], video[f - 1] if prev else None, bwd[f - 1] if prev else None,
                                  video[f + 1] if nxt else None, fwd[f] if nxt else None, thr, px, py, window)


def test_chain_filters_every_slot_and_batch_one_side(bbme):
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    fields = _video_fields(bbme, "chain", video)
    chain = bbme.MFChain(video, search, block)
    chain.estimate_bidirectional_async()
    for p in range(4):
        assert np.array_equal(chain.get_pair_cells(p), fields[0][p]) and np.array_equal(chain.get_pair_backward_cells(p), fields[1][p])
    CH, CW = chain.cells_shape
    win = odd_windows(CH, CW)[1]
    for thr in (64, 1021):
        exp = [_video_rule(video, fields, f, thr)[0] for f in range(5)]
        run = chain.temporal_filter_run_bgr(thr)
        assert run.shape == (5, VIDEO[1], VIDEO[0], 3)
        for f in range(5):
            assert np.array_equal(run[f], exp[f]), (thr, f)
        assert np.array_equal(chain.temporal_filter_run_bgr(thr, 1, 3), np.stack(exp[1:4]))      # a sub-run from one launch
        assert np.array_equal(chain.temporal_filter_run_bgr(thr, 4, 1)[0], exp[4])
        for p in range(4):
            assert np.array_equal(chain.get_frame_filtered_bgr(p, 0, thr), exp[p]), (thr, p)
            assert np.array_equal(chain.get_frame_filtered_bgr(p, 1, thr), exp[p + 1]), (thr, p)  # (p, 1) and (p + 1, 0): one frame
        assert np.array_equal(chain.temporal_filter_bgr(thr), exp[0])
        for w, np_win in ((None, chain.default_cell_window()), ("all", None), (win, win)):
            assert [_stats(s) for s in chain.temporal_filter_bgr_stats(thr, w)] == \
                [_video_rule(video, fields, f, thr, np_win)[2] for f in range(5)], (thr, w)
    inner = _video_rule(video, fields, 2, 64)
    assert (inner[1] & 0x0f).any() and (inner[1] >> 4).any()                       # inner frames take from both sides
    for p, w in ((0, 0), (1, 1), (3, 1)):
        assert np.array_equal(chain.frame_bgr_tensor(p, w).cpu().numpy(), video[p + w])
    chain.close()
    # a batch of the same pairs: every frame one-sided
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(4)], search, block)
    batch.estimate_bidirectional_async()
    for p in range(4):
        assert np.array_equal(batch.get_frame_filtered_bgr(p, 0, 64), _video_rule(video, fields, p, 64, side="next")[0]), p
        assert np.array_equal(batch.get_frame_filtered_bgr(p, 1, 64), _video_rule(video, fields, p + 1, 64, side="prev")[0]), p
        assert np.array_equal(batch.frame_bgr_tensor(p, 1).cpu().numpy(), video[p + 1])
    for w, np_win in ((win, win), ("all", None)):
        exp = []
        for p in range(4):
            exp += [_video_rule(video, fields, p, 64, np_win, side="next")[2], _video_rule(video, fields, p + 1, 64, np_win, side="prev")[2]]
        assert [_stats(s) for s in batch.temporal_filter_bgr_stats(64, w)] == exp, w
    batch.close()


def test_colour_filter_needs_fields_and_stored_colour(bbme):
    from blockbasedmotionestimation_amd import _capi
    search, block = VIDEO_PARAMS
    video = colour_video(bbme)
    c1, c2 = video[:2]
    g1, g2 = np_bgr_to_gray(c1), np_bgr_to_gray(c2)
    state = _capi.ERR_STATE
    mf = bbme.MF(c1, c2, search, block)
    calls = (lambda: mf.temporal_filter_bgr(64), lambda: mf.temporal_filter_bgr(64, 1), lambda: mf.temporal_filter_bgr_stats(64))
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # no bidirectional estimate yet
    mf.estimate_async()
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # a forward estimate is none either
    mf.estimate_bidirectional_async()
    first, stats = mf.temporal_filter_bgr(64), mf.temporal_filter_bgr_stats(64)
    grey = mf.temporal_filter(64)
    mf.set_frames(g1, g2)                                  # a grey setter withdraws the colour
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter(64), grey)    # the same luma: the grey filter stands
    assert [_status(bbme, c) for c in calls] == [state] * 3
    assert _status(bbme, lambda: mf.frame_bgr_tensor(0, 0)) == state
    mf.set_frames(c1, c2)
    assert [_status(bbme, c) for c in calls] == [state] * 3                        # colour again, but no fields
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.temporal_filter_bgr(64), first) and mf.temporal_filter_bgr_stats(64) == stats
    mf.close()
    # a context that never saw a colour setter has no colour store at all
    mf = bbme.MF(g1, g2, search, block)
    mf.estimate_bidirectional_async()
    assert [_status(bbme, c) for c in (lambda: mf.temporal_filter_bgr(64), lambda: mf.temporal_filter_bgr_stats(64))] == [state] * 2
    mf.close()
    # a chain: a grey setter of ONE slot withdraws the frames that read it (the slot and its two neighbours), and no other
    chain = bbme.MFChain(video, search, block)
    chain.estimate_bidirectional_async()
    run = chain.temporal_filter_run_bgr(64)
    chain.set_frame_run(1, [np_bgr_to_gray(video[1])])
    chain.estimate_bidirectional_async()
    for p, w in ((0, 0), (0, 1), (1, 1)):                  # slots 0, 1, 2
        assert _status(bbme, lambda: chain.get_frame_filtered_bgr(p, w, 64)) == state, (p, w)
    assert _status(bbme, lambda: chain.temporal_filter_run_bgr(64)) == state
    assert _status(bbme, lambda: chain.temporal_filter_run_bgr(64, 2, 3)) == state
    assert _status(bbme, lambda: chain.temporal_filter_bgr_stats(64)) == state
    assert np.array_equal(chain.get_frame_filtered_bgr(2, 1, 64), run[3])          # slot 3 reads slots 2, 3, 4
    assert np.array_equal(chain.temporal_filter_run_bgr(64, 3, 2), run[3:5])
    chain.set_frame_run(1, [video[1]])
    assert _status(bbme, lambda: chain.temporal_filter_run_bgr(64)) == state       # slots set, not estimated
    chain.estimate_bidirectional_async()
    assert np.array_equal(chain.temporal_filter_run_bgr(64), run)
    chain.close()


def test_colour_filter_changes_no_state_and_refuses_bad_arguments(bbme):
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
                    flow=mf.get_pair_flow(1), grey=mf.temporal_filter_run(64), half=mf.interpolate_bgr(1, 2, pair=1))

    def same(a, b):
        assert a.keys() == b.keys()
        for k in a:
            for x, y in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]):
                assert np.array_equal(x, y), k

    before = state()
    frames = [mf.frame_bgr_tensor(p, w_).clone() for p, w_ in ((0, 0), (0, 1), (1, 1))]
    gp, gn = mf.backward_cells_tensor(0).clone(), mf.cells_tensor(1).clone()
    out = torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda")
    wmap = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    run = mf.temporal_filter_run_bgr(64)
    stats = mf.temporal_filter_bgr_stats(64, "all")
    mf.cells_temporal_filter_bgr_device(frames[1], frames[0], frames[2], gp, gn, 64, out=out[0], weights=wmap, stats=st)
    mf.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), run[1]) and tuple(st.cpu().tolist()) == _stats(stats[1])
    # the other getters' scratch buffers and the filter's are independent
    mf.temporal_filter_stats(64, "all")
    mf.get_frame_filtered(0, 1, 64)
    mf.interpolate_bgr(1, 3)
    assert np.array_equal(mf.temporal_filter_run_bgr(64), run) and mf.temporal_filter_bgr_stats(64, "all") == stats
    same(before, state())
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    buf = np.zeros((h, w, 3), np.uint8)
    s12 = (C.c_ulonglong * 12)()
    c_, p_, n_, gp_, gn_, o_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (frames[1], frames[0], frames[2], gp, gn, out, wmap, st))

    def cells(p=p_, c=c_, n=n_, bp=3 * w, a=gp_, b=gn_, thr=64, win=None, o=o_, op=3 * w, m=m_, mp=CW, s=s_):
        return L.bbme_cells_temporal_filter_bgr_device(ctx, p, c, n, bp, a, b, thr, win, o, op, m, mp, s, None)

    def own(pair=0, which=0, thr=64, o=o_, op=3 * w):
        return L.bbme_temporal_filter_bgr_device(ctx, pair, which, thr, o, op, None)

    def run_of(first=0, count=3, thr=64, o=o_, op=3 * w, os=3 * h * w):
        return L.bbme_temporal_filter_bgr_chain_device(ctx, first, count, thr, o, op, os, None)

    def host(pair=0, which=0, thr=64, o=buf.ctypes.data):
        return L.bbme_get_temporal_filtered_bgr_host(ctx, pair, which, thr, o)

    assert cells() == 0 and own() == 0 and run_of() == 0 and host() == 0
    assert cells(p=None, a=None) == 0 and cells(n=None, b=None) == 0
    assert cells(p=None, a=None, n=None, b=None) == inv                          # no neighbour at all
    assert cells(p=None) == inv and cells(a=None) == inv and cells(n=None) == inv and cells(b=None) == inv
    assert cells(c=None) == inv
    assert cells(o=None, m=None, s=None) == inv                                  # nothing asked for
    for frame in (c_, p_, n_):                                                   # an output inside an input frame
        assert cells(o=frame) == inv
    assert cells(o=C.c_void_p(c_.value + 3 * w)) == inv and cells(n=None, b=None, o=n_) == 0
    assert cells(o=None) == 0 and cells(m=None) == 0 and cells(s=None) == 0 and cells(o=None, m=None) == 0
    assert own(o=None) == inv and run_of(o=None) == inv and host(o=None) == inv
    assert L.bbme_temporal_filter_bgr_stats(ctx, 64, None, None) == inv
    for thr in (0, -5, 1022):
        assert cells(thr=thr) == inv and own(thr=thr) == inv and run_of(thr=thr) == inv and host(thr=thr) == inv, thr
        assert L.bbme_temporal_filter_bgr_stats(ctx, thr, None, s12) == inv
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
        assert L.bbme_temporal_filter_bgr_stats(ctx, 64, w4, s12) == inv, win
    assert L.bbme_temporal_filter_bgr_stats(ctx, 64, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s12) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_bgr_device(frames[1], frames[0], None, gp[:, :CW - 2], None, 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_temporal_filter_bgr_device(frames[1], frames[0][:, :w - 1], None, gp, None, 64, out=out[0])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.temporal_filter_run_bgr(64, 2, 3)
    assert e.value.status == inv
    mf.synchronize()
    same(before, state())
    assert np.array_equal(mf.temporal_filter_run_bgr(64), run)
    mf.close()
    # the chain call on anything but a chain
    pair = bbme.MF(video[0], video[1], search, block)
    pair.estimate_bidirectional_async()
    assert L.bbme_temporal_filter_bgr_chain_device(pair._ctx, 0, 1, 64, o_, 3 * w, 0, None) == _capi.ERR_UNSUPPORTED
    # the entry point that takes frames and grids needs neither frames nor fields nor stored colour
    ctx2 = C.c_void_p()
    params = _capi.make_params(search, block)
    assert L.bbme_create(C.byref(params), w, h, 0, C.byref(ctx2)) == 0
    z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    cur = torch.full((h, w, 3), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.bbme_cells_temporal_filter_bgr_device(ctx2, None, C.c_void_p(cur.data_ptr()), C.c_void_p(cur.data_ptr()), 3 * w, None,
                                                   C.c_void_p(z.data_ptr()), 64, None, o_, 3 * w, None, 0, None, None) == 0
    assert L.bbme_synchronize(ctx2) == 0
    assert bool((out[0] == 9).all())
    assert L.bbme_temporal_filter_bgr_device(ctx2, 0, 0, 64, o_, 3 * w, None) == _capi.ERR_STATE
    assert L.bbme_destroy(ctx2) == 0
    pair.close()


def _colour7(bbme):
    """Seven colour frames: colour_video's three pointwise maps of a seven-frame video."""
    if "video7" not in _cache:
        grey = bbme.synth_video(VIDEO[0], VIDEO[1], 7, VIDEO[3], max_motion=VIDEO[4])
        _cache["video7"] = [np.ascontiguousarray(np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1))
                            for v in grey]
    return _cache["video7"]


@pytest.mark.parametrize("in_flight,batch", [(4, 2), (1, 1)])
def test_denoise_frames_in_colour(bbme, in_flight, batch):
    """in_flight=4, batch=2: two contexts, a carried round each and the segment boundary at frame 3."""
    from blockbasedmotionestimation_amd.sequence import denoise_frames
    search, block = VIDEO_PARAMS
    video = _colour7(bbme)
    fields = _video_fields(bbme, "denoise", video)
    if "denoise_exp" not in _cache:
        _cache["denoise_exp"] = [_video_rule(video, fields, f, 96)[0] for f in range(7)]
    exp = _cache["denoise_exp"]
    keep = [v.copy() for v in video]
    got = denoise_frames(video, search, block, 96, in_flight=in_flight, batch=batch)
    assert len(got) == 7
    for v, k in zip(video, keep):
        assert np.array_equal(v, k)
    for f in range(7):
        assert got[f].shape == (VIDEO[1], VIDEO[0], 3) and got[f].dtype == np.uint8
        assert np.array_equal(got[f], exp[f]), f
    assert any(not np.array_equal(got[f], video[f]) for f in range(7))


def test_cli_writes_the_denoised_colour_frames(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    video = colour_video(bbme)
    c1, c2 = (np.ascontiguousarray(v[:72, :96]) for v in video[:2])
    _write_ppm(tmp_path / "f1.ppm", c1)
    _write_ppm(tmp_path / "f2.ppm", c2)
    args = ["--levels", "3", "--block", "16", "--search", "30", "--no-upsample", "--strength", "96"]
    r = subprocess.run([_build.CLI, str(tmp_path / "f1.ppm"), str(tmp_path / "f2.ppm")] + args + ["--denoise", str(tmp_path / "dn")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(c1, c2, [30] * 3, [16] * 3)
    mf.estimate_bidirectional_async()
    px, py = mf.padding_x, mf.padding_y
    for which in (0, 1):
        frame = mf.temporal_filter_bgr(96, which)
        assert (tmp_path / ("dn_%d.ppm" % (which + 1))).read_bytes() == \
            b"P6\n96 72\n255\n" + np.ascontiguousarray(frame[..., ::-1]).tobytes(), which
        luma = mf.temporal_filter(96, which)[py:py + 72, px:px + 96]
        assert (tmp_path / ("dn_%d.pgm" % (which + 1))).read_bytes() == b"P5\n96 72\n255\n" + luma.tobytes(), which
    mf.close()
    # grey frames: the luma files alone
    for name, c in (("g1.pgm", c1), ("g2.pgm", c2)):
        g = np_bgr_to_gray(c)
        (tmp_path / name).write_bytes(b"P5\n96 72\n255\n" + g.tobytes())
    r = subprocess.run([_build.CLI, str(tmp_path / "g1.pgm"), str(tmp_path / "g2.pgm")] + args + ["--denoise", str(tmp_path / "gr")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "gr_1.pgm").exists() and (tmp_path / "gr_2.pgm").exists()
    assert not (tmp_path / "gr_1.ppm").exists() and not (tmp_path / "gr_2.ppm").exists()
    assert (tmp_path / "gr_1.pgm").read_bytes() == (tmp_path / "dn_1.pgm").read_bytes()          # the luma of the colour run
