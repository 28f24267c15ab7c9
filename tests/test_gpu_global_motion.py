"""K16 k_vector_histogram, K17 k_global_moments and K18 k_global_compensate against the numpy restatements of the GLOBAL MOTION
RULE and the GLOBAL COMPENSATION RULE (tests/test_global_motion_cpu.py), bit for bit, on injected grids and planes; the context's
own estimate against the CPU route on the downloaded cells and mask, on every kind of context; the context-level compensation;
refusals and state, the refusal of planes beyond 8188 among them; the deepest batch; up-sampled and colour contexts; the guard
bands; sequence.stabilize_frames.  (The kernels at 2 Mpixel and at the rule's largest planes: tests/test_gpu_scale.py.)"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _cuda, _stats_of
from test_global_motion_cpu import (BINS, COMP_MODELS, MODELS, STAT_KEYS, cutting_windows, extreme_grid, np_global_compensate,
                                    np_histogram, np_moments, plane_windows, random_grid, random_mask, uniform_grid)

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

PATTERN = 0x5A


def _grid_tensors(mf, g, excl, q_extra, e_extra):
    """A grid whose rows are q_extra cells further apart than packed and a mask whose rows are e_extra bytes further apart"""
    import torch
    CH, CW = mf.cells_shape
    tq = torch.full((CH, CW + q_extra, 2), 0x7777, dtype=torch.int16, device="cuda")
    tq[:, :CW] = _cuda(np.asarray(g, np.int16))
    te = None
    if excl is not None:
        te = torch.full((CH, CW + e_extra), 0xEE, dtype=torch.uint8, device="cuda")
        te[:, :CW] = _cuda(np.asarray(excl, np.uint8))
        te = te[:, :CW]
    return tq[:, :CW], te


def _finish(mf, stream):
    if stream is not None:
        stream.synchronize()
    mf.synchronize()


def _hist(mf, g, excl=None, window=None, q_extra=0, e_extra=0, stream=None, twice=False):
    import torch
    tq, te = _grid_tensors(mf, g, excl, q_extra, e_extra)
    hist = torch.full((2, BINS), 12345, dtype=torch.int32, device="cuda")             # the call zeroes the table itself
    torch.cuda.synchronize()
    for _ in range(2 if twice else 1):
        mf.cells_vector_histogram_device(tq, hist, te, window, None if stream is None else stream.cuda_stream)
    _finish(mf, stream)
    return hist.cpu().numpy().astype(np.uint32)


def _moments(mf, g, model, tol, excl=None, window=None, want=("map", "words"), map_offset=0, map_extra=0, q_extra=0, e_extra=0,
             stream=None):
    """-> (map, words), None where not asked for; the map is a column slice of a wider tensor with two more rows, and nothing
    outside its rectangle may change"""
    import torch
    CH, CW = mf.cells_shape
    tq, te = _grid_tensors(mf, g, excl, q_extra, e_extra)
    whole = torch.full((CH + 2, CW + map_offset + map_extra), PATTERN, dtype=torch.uint8, device="cuda") if "map" in want else None
    tmap = None if whole is None else whole[1:CH + 1, map_offset:map_offset + CW]
    words = torch.full((16,), -7, dtype=torch.int64, device="cuda") if "words" in want else None
    torch.cuda.synchronize()
    mf.cells_global_moments_device(tq, model, tol, te, tmap, words, window, None if stream is None else stream.cuda_stream)
    _finish(mf, stream)
    got_map = None
    if whole is not None:
        host = whole.cpu().numpy()
        got_map = host[1:CH + 1, map_offset:map_offset + CW].copy()
        host[1:CH + 1, map_offset:map_offset + CW] = PATTERN
        assert (host == PATTERN).all(), "bytes outside the map's rectangle changed"
    return got_map, None if words is None else words.cpu().numpy()


def _compensate(mf, I1, I2, model, unit, fill=0, window=None, want=("out", "stats"), out_offset=0, out_extra=0, stream=None):
    import torch
    H0, W0 = mf.padded_height, mf.padded_width
    t1, t2 = _cuda(I1), _cuda(I2)
    whole = torch.full((H0 + 2, W0 + out_offset + out_extra), PATTERN, dtype=torch.uint8, device="cuda") if "out" in want else None
    out = None if whole is None else whole[1:H0 + 1, out_offset:out_offset + W0]
    st = torch.zeros(4, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    mf.cells_global_compensate_device(t1 if st is not None else None, t2, model, unit, out, st, fill, window,
                                      None if stream is None else stream.cuda_stream)
    _finish(mf, stream)
    frame = None
    if whole is not None:
        host = whole.cpu().numpy()
        frame = host[1:H0 + 1, out_offset:out_offset + W0].copy()
        host[1:H0 + 1, out_offset:out_offset + W0] = PATTERN
        assert (host == PATTERN).all(), "bytes outside the frame's rectangle changed"
    return frame, None if st is None else tuple(st.cpu().tolist())


# 200 x 136 at [30] * 3 / [16] * 3 pads to 256 x 192: 128 cell columns, every cell row whole runs of 4.  132 x 100 at [12] / [2] is
# not padded: 66 cell columns, every cell row ends in a run of 2, and rows of 66 cells put every second one off 8-byte alignment
INJECTED = [(200, 136, [30] * 3, [16] * 3), (132, 100, [12], [2])]


def _injected_context(bbme, w, h, search, block):
    f1, f2, _ = bbme.synth_pair(w, h, 900 + w, max_motion=4, tiles=3)
    mf = bbme.MF(f1, f2, search, block)
    CH, CW = mf.cells_shape
    assert (mf.padded_width, CW % 4) == ((256, 0) if w == 200 else (132, 2))
    return mf


@pytest.mark.parametrize("w,h,search,block", INJECTED)
def test_histogram_and_moments_on_injected_grids(bbme, w, h, search, block):
    import torch
    mf = _injected_context(bbme, w, h, search, block)
    CH, CW = mf.cells_shape
    grids = (("random", random_grid(CH, CW, 1)), ("uniform", uniform_grid(CH, CW)), ("extreme", extreme_grid(CH, CW, 2)))
    mask = random_mask(CH, CW, 3)
    wins = cutting_windows(CW, CH)
    side = torch.cuda.Stream()
    for name, g in grids:
        # K16
        assert np.array_equal(_hist(mf, g), np_histogram(g)), name
        assert np.array_equal(_hist(mf, g, mask, wins[0], q_extra=5, e_extra=3, twice=True), np_histogram(g, mask, wins[0])), name
        assert np.array_equal(_hist(mf, g, mask, None, e_extra=3, stream=side), np_histogram(g, mask)), name
        for win in wins[1:]:
            assert np.array_equal(_hist(mf, g, None, win, q_extra=1), np_histogram(g, None, win)), (name, win)
        # K17
        for k, model in enumerate(MODELS):
            tol = (0, 65536, 3 * 65536, 2 ** 40, 65536)[k]
            win = wins[k % len(wins)]
            got = _moments(mf, g, model, tol, mask, win, map_offset=1 + k % 3, map_extra=2, q_extra=k, e_extra=3,
                           stream=side if k == 2 else None)
            exp = np_moments(g, model, tol, mask, win)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (name, model, tol, win, got[1], exp[1])
        model, tol = MODELS[2], 2 * 65536
        exp = np_moments(g, model, tol)
        got = _moments(mf, g, model, tol, want=("words",))
        assert got[0] is None and np.array_equal(got[1], exp[1]), (name, "words alone")
        got = _moments(mf, g, model, tol, want=("map",), map_extra=8)
        assert got[1] is None and np.array_equal(got[0], exp[0]), (name, "map alone")
    # everything excluded: n = 0 and n2 alone
    everything = np.ones((CH, CW), np.uint8)
    assert _hist(mf, grids[0][1], everything).sum() == 0
    assert _moments(mf, grids[0][1], MODELS[1], 65536, everything)[1].tolist() == [0, 0, CH * CW] + [0] * 13
    # refusals
    tq, te = _grid_tensors(mf, grids[0][1], mask, 0, 0)
    hist = torch.zeros((2, BINS), dtype=torch.int32, device="cuda")
    words = torch.zeros(16, dtype=torch.int64, device="cuda")
    tmap = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    bad = (lambda: mf.cells_vector_histogram_device(tq, hist, window=(0, 0, CW + 1, 1)),
           lambda: mf.cells_vector_histogram_device(tq, hist[:1]),
           lambda: mf.cells_vector_histogram_device(tq[:, :CW - 1], hist),
           lambda: mf.cells_global_moments_device(tq, MODELS[0], 65536),
           lambda: mf.cells_global_moments_device(tq, MODELS[0], -1, words=words),
           lambda: mf.cells_global_moments_device(tq, MODELS[0], 2 ** 40 + 1, words=words),
           lambda: mf.cells_global_moments_device(tq, MODELS[0][:5], 0, words=words),
           lambda: mf.cells_global_moments_device(tq, MODELS[0], 0, map=tmap[:, :CW - 1]),
           lambda: mf.cells_global_moments_device(tq, MODELS[0], 0, words=words[:15]),
           lambda: mf.cells_global_moments_device(tq, MODELS[0], 0, words=words, window=(-1, 0, 2, 2)))
    for k, call in enumerate(bad):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == -1, k
    mf.close()


@pytest.mark.parametrize("w,h,search,block", INJECTED)
def test_compensation_on_injected_planes(bbme, w, h, search, block):
    import torch
    mf = _injected_context(bbme, w, h, search, block)
    W0, H0 = mf.padded_width, mf.padded_height
    rng = np.random.default_rng(w)
    I1, I2 = rng.integers(0, 256, size=(2, H0, W0)).astype(np.uint8)
    wins = [None] + plane_windows(W0, H0)
    side = torch.cuda.Stream()
    skipped_all = 0
    for k, (model, unit) in enumerate(COMP_MODELS):
        fill, win = (0, 7, 255)[k % 3], wins[k % len(wins)]
        frame, st = _compensate(mf, I1, I2, model, unit, fill, win, out_offset=k % 4, out_extra=(3, 0, 8)[k % 3],
                                stream=side if k == 1 else None)
        exp = np_global_compensate(I1, I2, model, unit, fill, win)
        assert np.array_equal(frame, exp[0]), (model, unit, np.argwhere(frame != exp[0])[:4])
        assert st == exp[1], (model, unit, win, st, exp[1])
        skipped_all += exp[1][2] == 0
    assert skipped_all >= 2                                              # models that skip everything
    model, unit = COMP_MODELS[1]
    exp = np_global_compensate(I1, I2, model, unit, 9, wins[1])
    assert _compensate(mf, I1, I2, model, unit, 9, wins[1], want=("stats",)) == (None, exp[1])
    frame, st = _compensate(mf, None, I2, model, unit, 9, want=("out",), out_offset=5)
    assert st is None and np.array_equal(frame, exp[0])
    # the whole-pixel property
    for unit, (tx, ty) in ((1, (3, -2)), (4, (-5, 7))):
        frame, _ = _compensate(mf, None, I2, (tx * unit << 16, 0, 0, ty * unit << 16, 0, 0), unit, 77, want=("out",))
        ys, xs = np.mgrid[0:H0, 0:W0]
        ok = (ys + ty >= 0) & (ys + ty < H0) & (xs + tx >= 0) & (xs + tx < W0)
        exp = np.full((H0, W0), 77, np.uint8)
        exp[ok] = I2[(ys + ty)[ok], (xs + tx)[ok]]
        assert np.array_equal(frame, exp), (unit, tx, ty)
    # the largest sums: every pixel differs by 255
    _, st = _compensate(mf, np.zeros_like(I1), np.full_like(I1, 255), (0,) * 6, 1, want=("stats",))
    assert st == (255 * 255 * W0 * H0, 255 * W0 * H0, W0 * H0, 0)
    t1, t2 = _cuda(I1), _cuda(I2)
    out = torch.zeros((H0, W0), dtype=torch.uint8, device="cuda")
    st4 = torch.zeros(4, dtype=torch.int64, device="cuda")
    for kw in (dict(), dict(out=out, fill=256), dict(out=out, unit=2), dict(stats=st4, window=(0, 0, W0 + 1, 1)), dict(out=t2),
               dict(out=out[:, :W0 - 2]), dict(out=out, stats=st4[:3])):
        with pytest.raises(bbme.BbmeError) as e:
            mf.cells_global_compensate_device(t1, t2, COMP_MODELS[0][0], **kw)
        assert e.value.status == -1, kw
    with pytest.raises(bbme.BbmeError) as e:               # statistics need image 1
        mf.cells_global_compensate_device(None, t2, COMP_MODELS[0][0], stats=st4)
    assert e.value.status == -1
    mf.close()


# ---- the context's own estimate --------------------------------------------------------------------------------------------------
VARIANTS = [dict(which="forward"), dict(which="backward"), dict(which="forward", subpel=True, kind="translation"),
            dict(which="backward", subpel=True, mask_tol=1), dict(which="forward", mask_tol=1, iterations=0),
            dict(which="forward", mask_tol=1, tol=0.5, iterations=8)]


def _cpu_route(bbme, ctx, pair, which="forward", subpel=False, kind="affine", tol=1.0, iterations=3, mask_tol=None, window=None):
    """global_motion_cells on the downloaded cells and mask of `pair` -> (model, words, map)"""
    single = not hasattr(ctx, "batch")
    if subpel:
        cells = ctx.subpel_cells(which) if single else ctx.get_pair_subpel_cells(pair, which)
    elif which == "forward":
        cells = ctx.get_cells() if single else ctx.get_pair_cells(pair)
    else:
        cells = ctx.get_backward_cells() if single else ctx.get_pair_backward_cells(pair)
    excl = None if mask_tol is None else ctx.consistency(which, mask_tol, pair=pair)
    unit = 4 if subpel else 1
    return bbme.global_motion_cells(cells, kind, int(round(tol * unit * 65536)), iterations, excl,
                                    ctx.default_cell_window() if window is None else window)


def _assert_equals_cpu_route(bbme, ctx, pair, got, **kw):
    model, words, cls = _cpu_route(bbme, ctx, pair, **kw)
    assert np.array_equal(got["model"], model), (pair, kw, got["model"], model)
    assert [got["statistics"][k] for k in got["statistics"]] == words.tolist(), (pair, kw)
    assert got["unit"] == (4 if kw.get("subpel") else 1)
    if "map" in got:
        assert np.array_equal(got["map"], cls), (pair, kw)
    return model


def _state(mf):
    return [mf.get_cells(), mf.get_flow(), mf.get_backward_cells()]


def test_own_estimate_equals_the_cpu_route_and_changes_no_state(bbme):
    w, h, search, block = 200, 120, [20, 20], [8, 8]
    f1, f2, _ = bbme.synth_pair(w, h, 240, max_motion=5)
    mf = bbme.MF(f1, f2, search, block)
    with pytest.raises(bbme.BbmeError) as e:                  # before any estimate
        mf.global_motion()
    assert e.value.status == -7
    mf.calcMotionBlockMatching()
    for kw in (dict(which="backward"), dict(mask_tol=1)):     # both need a bidirectional estimate
        with pytest.raises(bbme.BbmeError) as e:
            mf.global_motion(**kw)
        assert e.value.status == -7, kw
    _assert_equals_cpu_route(bbme, mf, 0, mf.global_motion(), which="forward")
    mf.estimate_bidirectional_async()
    before = _state(mf)
    models = []
    for kw in VARIANTS:
        got = mf.global_motion(**kw)
        models.append(_assert_equals_cpu_route(bbme, mf, 0, got, **kw))
        assert got["statistics"]["inliers"] + got["statistics"]["outliers"] + got["statistics"]["excluded"] == \
            mf.default_cell_window()[2] * mf.default_cell_window()[3]
    odd = (3, 1, mf.cells_shape[1] - 7, mf.cells_shape[0] - 4)
    _assert_equals_cpu_route(bbme, mf, 0, mf.global_motion(window=odd), window=odd)
    _assert_equals_cpu_route(bbme, mf, 0, mf.global_motion(window="all"), window=(0, 0) + mf.cells_shape[::-1])
    assert models[4][1] == 0 and not np.array_equal(models[0], models[1])
    # the context-level compensation along the fitted model, and its statistics
    I1, I2 = mf.get_level_planes(0)
    win = (mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height)
    for which, a, b, model, unit in (("forward", I1, I2, models[0], 1), ("backward", I2, I1, models[3], 4)):
        exp = np_global_compensate(a, b, model, unit, 9, win)
        assert np.array_equal(mf.draw_MVimage_global(model, unit, which, 9), exp[0]), which
        assert _stats(mf.compensation_error_global(model, unit, which)) == exp[1], which
        host = bbme.global_compensate(a, b, model, unit, 9, win)
        assert np.array_equal(host[0], exp[0]) and _stats(host[1]) == exp[1]
    after = _state(mf)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))            # no state changed
    bad = (lambda: mf.global_motion(which=2), lambda: mf.global_motion(kind="similarity"), lambda: mf.global_motion(iterations=9),
           lambda: mf.global_motion(iterations=-1), lambda: mf.global_motion(tol=-1.0), lambda: mf.global_motion(tol=2.0 ** 25),
           lambda: mf.global_motion(window=(0, 0, mf.cells_shape[1] + 1, 1)), lambda: mf.draw_MVimage_global(models[0], 3),
           lambda: mf.draw_MVimage_global(models[0], 1, "forward", 256), lambda: mf.draw_MVimage_global(models[0][:4]),
           lambda: mf.compensation_error_global(models[0], 1, "forward", (0, 0, mf.padded_width + 1, 2)))
    for k, call in enumerate(bad):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == -1, k
    # direction BACKWARD: what a context fed the exchanged pair gives
    mf.set_direction(True)
    mf.calcMotionBlockMatching()
    got = mf.global_motion()
    _assert_equals_cpu_route(bbme, mf, 0, got, which="forward")
    frame = mf.draw_MVimage_global(got["model"])
    mf.close()
    swapped = bbme.MF(f2, f1, search, block)
    swapped.calcMotionBlockMatching()
    other = swapped.global_motion()
    assert np.array_equal(got["model"], other["model"]) and got["statistics"] == other["statistics"]
    assert np.array_equal(got["map"], other["map"]) and np.array_equal(frame, swapped.draw_MVimage_global(other["model"]))
    swapped.close()


def test_batch_and_chain_equal_single_contexts(bbme):
    w, h, search, block = 136, 104, [20, 20], [8, 8]
    frames = bbme.synth_video(w, h, 4, 21, max_motion=4)
    pairs = [(frames[p], frames[p + 1]) for p in range(3)]
    variants = [VARIANTS[0], VARIANTS[3], VARIANTS[5]]
    single = []
    for a, b in pairs:
        mf = bbme.MF(a, b, search, block)
        mf.estimate_bidirectional_async()
        got = [mf.global_motion(**kw) for kw in variants]
        m = got[0]["model"]
        single.append(dict(got=got, frame=mf.draw_MVimage_global(m, 1, "backward", 5), err=mf.compensation_error_global(m)))
        mf.close()
    assert len({tuple(s["got"][0]["model"]) for s in single}) == 3
    for ctx in (bbme.MFBatch(pairs, search, block), bbme.MFChain(frames, search, block)):
        ctx.estimate_bidirectional_async()
        cells = [ctx.get_pair_cells(p) for p in range(3)]
        for k, kw in enumerate(variants):
            got = ctx.global_motion_all(maps=True, **kw)
            for p in range(3):
                _assert_equals_cpu_route(bbme, ctx, p, got[p], **kw)
                exp = single[p]["got"][k]
                assert np.array_equal(got[p]["model"], exp["model"]) and got[p]["statistics"] == exp["statistics"], (p, kw)
                assert np.array_equal(got[p]["map"], exp["map"]), (p, kw)
        models = np.stack([s["got"][0]["model"] for s in single])
        assert ctx.compensation_errors_global(models) == [s["err"] for s in single]
        for p in (2, 0, 1):
            assert np.array_equal(ctx.get_pair_global_compensated(p, models[p], 1, "backward", 5), single[p]["frame"]), p
        assert all(np.array_equal(ctx.get_pair_cells(p), cells[p]) for p in range(3))
        ctx.close()


def test_planes_beyond_8188_are_refused_and_nothing_is_written(bbme):
    """8190 x 130 pads to 8192 x 132: every device call of the rule and the context's own estimate answer ERR_UNSUPPORTED before
    anything is launched"""
    import torch
    from blockbasedmotionestimation_amd import _capi
    z = np.zeros((130, 8190), np.uint8)
    mf = bbme.MF(z, z, [12], [4])
    assert (mf.padded_width, mf.padded_height) == (8192, 132)
    CH, CW = mf.cells_shape
    cells = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    hist = torch.full((2, BINS), 12345, dtype=torch.int32, device="cuda")
    words = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    tmap = torch.full((CH, CW), PATTERN, dtype=torch.uint8, device="cuda")
    plane = torch.zeros((2 * CH, 2 * CW), dtype=torch.uint8, device="cuda")
    out = torch.full((2 * CH, 2 * CW), PATTERN, dtype=torch.uint8, device="cuda")
    st = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    calls = (lambda: mf.cells_vector_histogram_device(cells, hist),
             lambda: mf.cells_global_moments_device(cells, MODELS[1], 65536, map=tmap, words=words),
             lambda: mf.cells_global_compensate_device(plane, plane, COMP_MODELS[0][0], 1, out, st),
             lambda: mf.global_motion(),
             lambda: mf.draw_MVimage_global(COMP_MODELS[0][0]),
             lambda: mf.compensation_error_global(COMP_MODELS[0][0]))
    for k, call in enumerate(calls):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == _capi.ERR_UNSUPPORTED == -8, k
    mf.synchronize()
    torch.cuda.synchronize()
    assert (hist == 12345).all() and (words == -7).all() and (tmap == PATTERN).all() and (out == PATTERN).all() and (st == -7).all()
    mf.close()


def test_deepest_batch_equals_the_cpu_route_for_every_pair(bbme):
    """BBME_MAX_BATCH = 64 pairs behind every launch of the estimate (blockIdx.y of K16, K17 and K18, 64 rows of the model table)"""
    w, h, search, block = 72, 56, [12, 12], [8, 8]
    base = [bbme.synth_pair(w, h, 7300 + i, max_motion=2 + i % 4)[:2] for i in range(16)]
    pairs = []
    for k in range(64):                                        # sixteen distinct pairs and the same pairs rolled: distinct content
        f1, f2 = base[k % 16]
        sh = (2 * (k // 16), 3 * (k // 16))
        pairs.append((np.ascontiguousarray(np.roll(f1, sh, (0, 1))), np.ascontiguousarray(np.roll(f2, sh, (0, 1)))))
    mb = bbme.MFBatch(pairs, search, block)
    assert mb.batch == 64
    mb.estimate_bidirectional_async()
    kw = VARIANTS[3]
    got = mb.global_motion_all(maps=True, **kw)
    assert len(got) == 64
    models = np.stack([_assert_equals_cpu_route(bbme, mb, p, got[p], **kw) for p in range(64)])
    assert not np.array_equal(models[0], models[63]) and len({tuple(m) for m in models}) >= 16
    win = (mb.padding_x, mb.padding_y, mb.orig_width, mb.orig_height)
    errs = mb.compensation_errors_global(models, 4, "backward")
    for p in range(64):
        I1, I2 = (mb.frame_plane_tensor(p, which).cpu().numpy() for which in (0, 1))
        assert _stats(errs[p]) == np_global_compensate(I2, I1, models[p], 4, 0, win)[1], p
    mb.close()


def _check_own_estimate(bbme, mf, variants):
    """global_motion, draw_MVimage_global and compensation_error_global of a context against the CPU route on its downloaded
    cells and planes"""
    mf.estimate_bidirectional_async()
    I1, I2 = mf.get_level_planes(0)
    win = (mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height)
    models = []
    for kw in variants:
        got = mf.global_motion(**kw)
        model = _assert_equals_cpu_route(bbme, mf, 0, got, **kw)
        which, unit = kw["which"], 4 if kw.get("subpel") else 1
        a, b = (I1, I2) if which == "forward" else (I2, I1)
        exp = np_global_compensate(a, b, model, unit, 9, win)
        assert np.array_equal(mf.draw_MVimage_global(model, unit, which, 9), exp[0]), kw
        assert _stats(mf.compensation_error_global(model, unit, which)) == exp[1], kw
        assert exp[1][2] > 0
        models.append(model)
    return models


def test_own_estimate_on_an_upsampled_context(bbme):
    f1, f2, _ = bbme.synth_pair(50, 34, 250, max_motion=2)
    mf = bbme.MF(f1, f2, [20, 20], [8, 8], upsample=4)
    assert (mf.orig_width, mf.orig_height, mf.source_width) == (200, 136, 50)
    I1, _ = mf.get_level_planes(0)
    py, px = mf.padding_y, mf.padding_x
    assert np.array_equal(I1[py:py + 136, px:px + 200], bbme.resize_x4(f1))           # the planes are the up-sampled frames
    models = _check_own_estimate(bbme, mf, (VARIANTS[0], VARIANTS[3], VARIANTS[5]))
    assert any(m.any() for m in models)
    mf.close()


def test_own_estimate_on_a_colour_context_keeps_its_colour(bbme):
    w, h = 200, 120
    f1, f2, _ = bbme.synth_pair(w, h, 251, max_motion=5)
    rng = np.random.default_rng(252)
    tint = rng.integers(0, 64, (h, w, 3)).astype(np.int64)
    c1 = np.clip(f1[:, :, None].astype(np.int64) + tint - 32, 0, 255).astype(np.uint8)
    c2 = np.clip(f2[:, :, None].astype(np.int64) + tint - 32, 0, 255).astype(np.uint8)
    mf = bbme.MF(c1, c2, [20, 20], [8, 8])
    py, px = mf.padding_y, mf.padding_x
    I1, _ = mf.get_level_planes(0)
    assert np.array_equal(I1[py:py + h, px:px + w], bbme.bgr_to_gray(c1))               # the planes are the luma of the colour
    models = _check_own_estimate(bbme, mf, (VARIANTS[0], VARIANTS[3], VARIANTS[5]))
    assert any(m.any() for m in models)
    # the stored colour is still there, and still the frames that were set
    frame = mf.draw_MVimage_global_bgr(models[0], 1, "forward", 9)
    assert np.array_equal(frame, bbme.global_compensate_bgr(None, c2, models[0], 1, 9, px, py)[0])
    assert np.array_equal(mf.frame_bgr_tensor(0, 0).cpu().numpy(), c1)
    mf.close()


# ---- guard bands ---------------------------------------------------------------------------------------------------------------
def _guarded_results(bbme):
    """The own-context calls of one single, one batch and one chain context and the three calls on injected buffers -> sha256"""
    w, h, search, block = 136, 104, [20, 20], [8, 8]
    frames = bbme.synth_video(w, h, 3, 5, max_motion=4)
    results = []
    mf = bbme.MF(frames[0], frames[1], search, block)
    mf.estimate_bidirectional_async()
    for kw in (VARIANTS[0], VARIANTS[3]):
        got = mf.global_motion(**kw)
        results += [got["model"], np.array(list(got["statistics"].values()), np.int64), got["map"]]
    model = results[0]
    results += [mf.draw_MVimage_global(model, 1, "forward", 1), np.array(_stats(mf.compensation_error_global(model)))]
    CH, CW = mf.cells_shape
    g, mask = extreme_grid(CH, CW, 4), random_mask(CH, CW, 5)
    results.append(_hist(mf, g, mask, (1, 1, CW - 3, CH - 2), q_extra=1, e_extra=3))
    results += list(_moments(mf, g, MODELS[2], 65536, mask, (1, 1, CW - 3, CH - 2), map_offset=1, map_extra=2))
    I1, I2 = mf.get_level_planes(0)
    results.append(_compensate(mf, I1, I2, COMP_MODELS[0][0], 1, 7, (1, 1, 9, 7), out_offset=1)[0])
    ctxs = [mf, bbme.MFBatch([(frames[0], frames[1]), (frames[1], frames[2])], search, block), bbme.MFChain(frames, search, block)]
    for ctx in ctxs[1:]:
        ctx.estimate_bidirectional_async()
        got = ctx.global_motion_all(maps=True, **VARIANTS[3])
        results += [np.stack([d["model"] for d in got]), got[1]["map"]]
        results.append(np.array([_stats(s) for s in ctx.compensation_errors_global(np.stack([d["model"] for d in got]), 4)]))
    return ctxs, hashlib.sha256(b"".join(np.ascontiguousarray(r).tobytes() for r in results)).hexdigest()


def _guard_child():
    """Runs in a fresh process under BBME_TEST_GUARD=1 and BBME_TEST_POISON=1: prints the digest of the results and the guards' state"""
    import ctypes as C
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    assert os.environ["BBME_TEST_GUARD"] == "1" and os.environ["BBME_TEST_POISON"] == "1"
    ctxs, digest = _guarded_results(bbme)
    live, violations, first = C.c_ulonglong(), C.c_ulonglong(), C.create_string_buffer(512)
    found = C.c_void_p()
    _capi.check(_capi.lib().bbme_test_guard_find(b"the global motion histograms", 1, C.byref(found)))
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
    for ctx in ctxs:
        ctx.close()
    after = C.c_ulonglong()
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(after), first, len(first)))
    print("GUARDED %s buffer=%d violations=%d after_close=%d %s" % (digest, bool(found.value), violations.value, after.value,
                                                                     first.value.decode()))


def test_guard_bands_and_poison(bbme):
    """The histograms, the model table, the moments scratch, the refined cells and the mask come from the context's allocation
    path: between guard bands and poisoned, the calls damage no band and give the bytes they give without the knobs."""
    ctxs, digest = _guarded_results(bbme)
    for ctx in ctxs:
        ctx.close()
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBME_TEST_GUARD="1", BBME_TEST_POISON="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_global_motion as t; t._guard_child()" % (tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:5] == [digest, "buffer=1", "violations=0", "after_close=0"], line[0]


# ---- stabilisation -------------------------------------------------------------------------------------------------------------
def _jitter_video(w, h, offsets, seed=12):
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, size=(h + 32, w + 32)).astype(np.float64)
    for _ in range(2):
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) / 4
    big = np.clip((big - big.mean()) * 3 + 128, 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(big[16 + oy:16 + oy + h, 16 + ox:16 + ox + w]) for ox, oy in offsets]


def test_stabilize_frames(bbme):
    from blockbasedmotionestimation_amd import sequence
    w, h, search, block = 96, 64, [16, 16], [8, 8]
    offsets = [(0, 0), (2, -1), (-1, 2), (3, 1), (1, -2)]
    video = _jitter_video(w, h, offsets)
    frames, models, corrections = sequence.stabilize_frames(video, search, block, radius=None, kind="translation")
    assert len(frames) == 5 and models.shape == (4, 6) and corrections.shape == (5, 6)
    # frame f shows the texture at offset o_f: its content moves by o_f - o_(f+1) from frame f to frame f + 1
    exp = np.array([[offsets[f][0] - offsets[f + 1][0], offsets[f][1] - offsets[f + 1][1]] for f in range(4)])
    assert np.array_equal(np.rint(models[:, [0, 3]] / 65536.0).astype(int), exp), models
    m = 8                                                                             # the interior: the jitter stays below it
    for f in range(5):
        assert frames[f].shape == (h, w)
        assert np.array_equal(frames[f][m:h - m, m:w - m], video[0][m:h - m, m:w - m]), f
    frames, models2, corrections = sequence.stabilize_frames(video, search, block, radius=1, kind="translation", fill=3)
    assert np.array_equal(models2, models)
    cum = np.concatenate([np.zeros((1, 6)), np.cumsum(models / 65536.0, axis=0)])      # translations add up
    exp = np.stack([cum[f] - cum[max(0, f - 1):min(5, f + 2)].mean(axis=0) for f in range(5)])
    assert np.array_equal(corrections, np.rint(exp * 65536.0).astype(np.int32))
    mf = bbme.MF(video[0], video[0], search, block)
    px, py = mf.padding_x, mf.padding_y
    mf.close()
    for f in range(5):
        padded = bbme.pad_zero(video[f], px, py)
        exp = bbme.global_compensate(None, padded, corrections[f], 1, 3)[0][py:py + h, px:px + w]
        assert np.array_equal(frames[f], exp), f
