"""K18b k_global_compensate_bgr against the host rule of the BGR GLOBAL COMPENSATION RULE (bbme_global_compensate_bgr_host, which
tests/test_global_compensation_bgr_cpu.py holds against numpy), bit for bit: caller's frames at odd pitches and the stored
colour, every output pitch and the byte path, runs of frames from one launch, a caller's stream; B = G = R contexts against the
grey calls; single, batched and chain contexts; refusals and state, planes beyond 8188 among them; a run of GC_MAX_FRAMES = 32
frames from one launch; the guard bands; sequence.stabilize_frames on a colour
video; bbme_cli --gm-out-bgr.  No tolerance appears."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _status
from test_bgr_cpu import SHAPES
from test_global_compensation_bgr_cpu import EDGE_MODEL, FILLS, frame_windows, models_for
from test_global_motion_cpu import STAT_KEYS

pytestmark = pytest.mark.gpu

PATTERN = 0x5A
GEOMETRIES = list(SHAPES)                                  # (w, h, search, block) -> pads (1,1), (1,0), (2,2), (0,0)
_cache = {}


def _frames(w, h, count=2, seed=0):
    rng = np.random.default_rng([w, h, seed])
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def _cases(bbme, geometry):
    """Per geometry, computed once: the two frames, the pads and per (model, unit) the fill, the window and the host rule's answer"""
    if geometry not in _cache:
        w, h = geometry[:2]
        px, py = SHAPES[geometry][2:]
        c1, c2 = _frames(w, h)
        windows = frame_windows(w, h)
        cases = []
        for n, (model, unit) in enumerate(models_for(w, h)):
            fill, window = FILLS[n % 3], windows[n % len(windows)]
            out, st = bbme.global_compensate_bgr(c1, c2, model, unit, fill, px, py, window)
            cases.append((model, unit, fill, window, out, tuple(st[k] for k in STAT_KEYS)))
        _cache[geometry] = (c1, c2, px, py, cases)
    return _cache[geometry]


def _pitched(frames, extra):
    """(N, H, W, 3) view of a buffer whose rows are `extra` bytes further apart than packed and whose frames 7 bytes further than
    their rows need; the gaps hold a pattern"""
    import torch
    n, (h, w) = len(frames), frames[0].shape[:2]
    pitch = 3 * w + extra
    stride = pitch * h + 7
    buf = torch.full((n * stride,), 0xC3, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (n, h, w, 3), (stride, pitch, 3, 1))
    view.copy_(torch.from_numpy(np.stack(frames)).cuda())
    return view


def _warp(mf, c1, c2, models, unit, fill=0, window=None, want=("out", "stats"), in_extra=0, out_extra=0, out_offset=0, stream=None,
          tensors=None):
    """cells_global_compensate_bgr_device on len(c2) frames -> (frames (N, H, W, 3) or None, [stats tuple per frame] or None).
    The output lies out_offset bytes into a buffer of PATTERN, rows out_extra bytes further apart than packed; nothing outside
    the frames' pixels may change.  tensors: (bgr1, bgr2) already in HBM instead of c1, c2."""
    import torch
    n = len(models)
    h, w = mf.orig_height, mf.orig_width
    if tensors is None:
        t2 = _pitched(c2, in_extra)
        t1 = _pitched(c1, in_extra) if "stats" in want else None
    else:
        t1, t2 = tensors
    pitch = 3 * w + out_extra
    stride = pitch * h + 5
    whole = torch.full((out_offset + n * stride + 16,), PATTERN, dtype=torch.uint8, device="cuda") if "out" in want else None
    out = None if whole is None else torch.as_strided(whole, (n, h, w, 3), (stride, pitch, 3, 1), out_offset)
    st = torch.full((4 * n,), -7, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    single = n == 1 and tensors is None
    mf.cells_global_compensate_bgr_device(None if t1 is None else (t1[0] if single else t1), t2[0] if single else t2,
                                          np.asarray(models, np.int32), unit, None if out is None else (out[0] if single else out), st,
                                          fill, window, None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    got = None
    if whole is not None:
        host = whole.cpu().numpy()
        view = np.lib.stride_tricks.as_strided(host[out_offset:], (n, h, w, 3), (stride, pitch, 3, 1))
        got = view.copy()
        view[...] = PATTERN
        assert (host == PATTERN).all(), "bytes outside the frames' pixels changed"
    return got, None if st is None else [tuple(st[4 * k:4 * k + 4].cpu().tolist()) for k in range(n)]


def _context(bbme, geometry, frames=None):
    w, h, search, block = geometry
    c1, c2 = frames if frames is not None else _frames(w, h)
    mf = bbme.MF(c1, c2, list(search), list(block))
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == SHAPES[geometry]
    return mf


# ---- parity with the host rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g[:2])
def test_cells_call_equals_the_host_rule(bbme, geometry):
    c1, c2, px, py, cases = _cases(bbme, geometry)
    mf = _context(bbme, geometry, (c1, c2))
    stored = (mf.frame_bgr_tensor(0, 0).unsqueeze(0), mf.frame_bgr_tensor(0, 1).unsqueeze(0))      # the context's own, pitch 3 W
    for n, (model, unit, fill, window, exp_out, exp_st) in enumerate(cases):
        kw = dict(in_extra=(1, 5)[n % 2], out_extra=(0, 1, 5)[n % 3], out_offset=n % 4)
        got, st = _warp(mf, [c1], [c2], [model], unit, fill, window, **kw)
        assert np.array_equal(got[0], exp_out), (model, unit, kw)
        assert st == [exp_st], (model, unit, window)
        got, st = _warp(mf, None, None, [model], unit, fill, window, out_extra=kw["out_extra"], out_offset=(n + 1) % 4, tensors=stored)
        assert np.array_equal(got[0], exp_out) and st == [exp_st], (model, unit, "stored colour")
        if n % 5 == 0:                                        # the frame alone (no frame 1) and the statistics alone
            got, none = _warp(mf, None, [c2], [model], unit, fill, None, want=("out",), out_offset=(n // 5) % 4, **{k: kw[k] for k in
                                                                                                                     ("in_extra", "out_extra")})
            assert none is None and np.array_equal(got[0], exp_out), (model, unit)
            none, st = _warp(mf, [c1], [c2], [model], unit, 255 - fill, window, want=("stats",), in_extra=kw["in_extra"])
            assert none is None and st == [exp_st], (model, unit)
    mf.close()


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g[:2])
def test_every_output_pitch_and_byte_offset(bbme, geometry):
    """Output pitches 3 W, 3 W + 1 and 3 W + 5 at base offsets 0..3 under the edge-straddling model: the dword path, the byte path
    and the rows that change between them"""
    c1, c2, px, py, cases = _cases(bbme, geometry)
    model, unit, fill, window, exp_out, exp_st = next(c for c in cases if (c[0], c[1]) == EDGE_MODEL)
    mf = _context(bbme, geometry)
    for out_extra in (0, 1, 5):
        for out_offset in (0, 1, 2, 3):
            for in_extra in (1, 5):
                got, st = _warp(mf, [c1], [c2], [model], unit, fill, window, in_extra=in_extra, out_extra=out_extra, out_offset=out_offset)
                assert np.array_equal(got[0], exp_out) and st == [exp_st], (out_extra, out_offset, in_extra)
    mf.close()


@pytest.mark.parametrize("geometry", GEOMETRIES[:3:2], ids=lambda g: "%dx%d" % g[:2])
def test_stored_colour_runs_of_frames_and_a_callers_stream(bbme, geometry):
    import torch
    w, h = geometry[:2]
    px, py = SHAPES[geometry][2:]
    c1, c2, _, _, cases = _cases(bbme, geometry)
    mf = _context(bbme, geometry, (c1, c2))
    # the stored colour of the context (pitch 3 W)
    s1, s2 = mf.frame_bgr_tensor(0, 0), mf.frame_bgr_tensor(0, 1)
    assert np.array_equal(s1.cpu().numpy(), c1) and np.array_equal(s2.cpu().numpy(), c2)
    for model, unit, fill, window, exp_out, exp_st in cases[::7]:
        got, st = _warp(mf, None, None, [model], unit, fill, window, out_extra=1, out_offset=3,
                        tensors=(s1.unsqueeze(0), s2.unsqueeze(0)))
        assert np.array_equal(got[0], exp_out) and st == [exp_st], (model, unit)
    # three frames under three different models from one launch = three single launches
    f1, f2 = _frames(w, h, 3, seed=1), _frames(w, h, 3, seed=2)
    window = (1, 2, w - 5, h - 3)
    stream = torch.cuda.Stream()
    for unit, models in ((1, [EDGE_MODEL[0], (3 << 16, 0, 0, -(2 << 16), 0, 0), (16384 + 3000, 300, 0, -8192, 0, -200)]),
                         (4, [tuple(4 * v for v in EDGE_MODEL[0]), (5 << 16, 0, 0, 7 << 16, 0, 0), (0, 0, 0, 0, 0, 0)])):
        host = [bbme.global_compensate_bgr(f1[k], f2[k], models[k], unit, 3, px, py, window) for k in range(3)]
        assert len({h_[1]["sse"] for h_ in host}) == 3
        for kw in (dict(in_extra=1, out_extra=5, out_offset=1), dict(in_extra=5, out_extra=0, out_offset=0, stream=stream)):
            got, st = _warp(mf, f1, f2, models, unit, 3, window, **kw)
            for k in range(3):
                one, st1 = _warp(mf, [f1[k]], [f2[k]], [models[k]], unit, 3, window, in_extra=kw["in_extra"])
                assert np.array_equal(got[k], host[k][0]) and np.array_equal(one[0], host[k][0]), (unit, k, kw)
                assert st[k] == st1[0] == tuple(host[k][1][s] for s in STAT_KEYS), (unit, k, kw)
        got, none = _warp(mf, None, f2, models, unit, 3, None, want=("out",), in_extra=1, stream=stream)
        assert all(np.array_equal(got[k], host[k][0]) for k in range(3))
    mf.close()


def test_a_run_of_32_frames_from_one_launch(bbme):
    """BBME_GC_MAX_FRAMES = 32 frames as blockIdx.y of one launch: 32 models in the caller's table, 32 statistics quadruples, the
    frames 5 bytes further apart than their rows need; 33 are refused"""
    w, h = 50, 38
    f1, f2 = _frames(w, h, 32, seed=3), _frames(w, h, 32, seed=4)
    mf = bbme.MF(f1[0], f2[0], [12], [4])
    px, py = mf.padding_x, mf.padding_y
    assert (mf.padded_width, mf.padded_height, px, py) == (52, 40, 1, 1)
    models = [(40000 * (k - 16), 40 * k, -25 * (k % 7), -30000 * (k % 11) + 90000, 30 * (k % 5), -45 * k) for k in range(32)]
    assert len(set(models)) == 32
    window = (1, 2, w - 5, h - 3)
    for unit in (1, 4):
        models = [tuple(unit * v + (unit == 4) for v in m) for m in models]               # the same motion in quarter pels, nearly
        host = [bbme.global_compensate_bgr(f1[k], f2[k], models[k], unit, 3, px, py, window) for k in range(32)]
        assert len({h_[1]["sse"] for h_ in host}) == 32 and len({h_[0].tobytes() for h_ in host}) == 32
        assert sum(h_[1]["skipped"] > 0 for h_ in host) >= 8
        got, st = _warp(mf, f1, f2, models, unit, 3, window, in_extra=1, out_extra=5, out_offset=1)      # (_warp checks the gaps)
        for k in range(32):
            assert np.array_equal(got[k], host[k][0]), (unit, k)
            assert st[k] == tuple(host[k][1][s] for s in STAT_KEYS), (unit, k, st[k], host[k][1])
    assert _status(bbme, lambda: _warp(mf, f1 + f1[:1], f2 + f2[:1], models + models[:1], 4, 3, window)) == -1
    mf.close()


def test_planes_beyond_8188_are_refused_and_nothing_is_written(bbme):
    """Frames of 8190 x 130 pad to 8192 x 132: ERR_UNSUPPORTED before anything is launched"""
    import torch
    from blockbasedmotionestimation_amd import _capi
    w, h = 8190, 130
    z = np.zeros((h, w, 3), np.uint8)
    mf = bbme.MF(z, z, [12], [4])
    assert (mf.padded_width, mf.padded_height) == (8192, 132)
    t = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((h, w, 3), PATTERN, dtype=torch.uint8, device="cuda")
    st = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    calls = (lambda: mf.cells_global_compensate_bgr_device(t, t, EDGE_MODEL[0], 1, out, st),
             lambda: mf.draw_MVimage_global_bgr(EDGE_MODEL[0]),
             lambda: mf.compensation_error_global_bgr(EDGE_MODEL[0]))
    for k, call in enumerate(calls):
        assert _status(bbme, call) == _capi.ERR_UNSUPPORTED == -8, k
    mf.synchronize()
    torch.cuda.synchronize()
    assert (out == PATTERN).all() and (st == -7).all()
    mf.close()


# ---- B = G = R: the grey calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES[:3], ids=lambda g: "%dx%d" % g[:2])
def test_grey_equivalence(bbme, geometry):
    w, h = geometry[:2]
    px, py = SHAPES[geometry][2:]
    rng = np.random.default_rng(w)
    g1, g2 = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    mf = _context(bbme, geometry, (np.repeat(g1[:, :, None], 3, 2), np.repeat(g2[:, :, None], 3, 2)))
    window = (2, 1, w - 7, h - 4)
    for model, unit in (EDGE_MODEL, ((851968 + 3, 2621, -1310, -393216, 1310, 2621), 4)):
        for which in ("forward", "backward"):
            grey = mf.draw_MVimage_global(model, unit, which, 9)
            colour = mf.draw_MVimage_global_bgr(model, unit, which, 9)
            assert colour.shape == (h, w, 3)
            for c in range(3):
                assert np.array_equal(colour[:, :, c], grey[py:py + h, px:px + w]), (which, c)
            gst = mf.compensation_error_global(model, unit, which, (window[0] + px, window[1] + py) + window[2:])
            cst = mf.compensation_error_global_bgr(model, unit, which, window)
            assert (cst["sse"], cst["sad"], cst["pixels"], cst["skipped"]) == (3 * gst["sse"], 3 * gst["sad"], gst["pixels"], gst["skipped"])
            assert cst["pixels"] > 0 and cst["mse"] == gst["mse"]
    mf.close()


# ---- context forms -------------------------------------------------------------------------------------------------------------
def test_context_forms_direction_state_and_refusals(bbme):
    geometry = GEOMETRIES[0]
    w, h, search, block = geometry
    search, block = list(search), list(block)
    px, py = SHAPES[geometry][2:]
    video = _frames(w, h, 4, seed=5)
    pairs = [(video[p], video[p + 1]) for p in range(3)]
    models = np.array([EDGE_MODEL[0], (3 << 16, 0, 0, -(2 << 16), 0, 0), (20000, -900, 400, 7000, -400, -900)], np.int32)
    window = (1, 0, w - 3, h - 1)
    host = {(p, which): bbme.global_compensate_bgr(*(pairs[p] if which == "forward" else pairs[p][::-1]), models[p], 1, 5, px, py, window)
            for p in range(3) for which in ("forward", "backward")}
    single = []
    for p, (a, b) in enumerate(pairs):
        mf = bbme.MF(a, b, search, block)
        mf.estimate_bidirectional_async()
        before = [mf.get_cells(), mf.get_flow(), mf.get_backward_cells()]
        for which in ("forward", "backward"):
            assert np.array_equal(mf.draw_MVimage_global_bgr(models[p], 1, which, 5), host[p, which][0]), (p, which)
            assert mf.compensation_error_global_bgr(models[p], 1, which, window) == host[p, which][1], (p, which)
        single.append(mf.compensation_error_global_bgr(models[p], 1, "forward", window))
        after = [mf.get_cells(), mf.get_flow(), mf.get_backward_cells()]
        assert all(np.array_equal(x, y) for x, y in zip(before, after))                # no state changed ...
        mf.calcMotionBlockMatching()
        assert np.array_equal(mf.get_cells(), before[0])                               # ... and a later estimate is the same
        if p == 0:
            # direction BACKWARD exchanges the frames
            mf.set_direction(True)
            assert np.array_equal(mf.draw_MVimage_global_bgr(models[0], 1, "forward", 5), host[0, "backward"][0])
            assert mf.compensation_error_global_bgr(models[0], 1, "forward", window) == host[0, "backward"][1]
            mf.set_direction(False)
            # refusals
            import torch
            t = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            narrow = torch.zeros((h, 3 * w - 1), dtype=torch.uint8, device="cuda")
            run = torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda")
            st = torch.zeros(4, dtype=torch.int64, device="cuda")
            lib, ctx, m = mf._lib, mf._ctx, models[0].ctypes.data
            cells = lib.bbme_cells_global_compensate_bgr_device
            bad = (lambda: mf.draw_MVimage_global_bgr(models[0], 3), lambda: mf.draw_MVimage_global_bgr(models[0], 1, "forward", 256),
                   lambda: mf.draw_MVimage_global_bgr(models[0][:4]), lambda: mf.draw_MVimage_global_bgr(models[0], 1, 2),
                   lambda: mf.compensation_error_global_bgr(models[0], 1, "forward", (0, 0, w + 1, 2)),
                   lambda: mf.compensation_error_global_bgr(models[0], 1, "forward", (0, 0, w, 0)),
                   lambda: mf.cells_global_compensate_bgr_device(None, t, models[0], 1),                       # neither out nor stats
                   lambda: mf.cells_global_compensate_bgr_device(None, t, models[0], 1, stats=st),             # stats without frame 1
                   lambda: mf.cells_global_compensate_bgr_device(None, t, models[:2], 1, out=t.clone()),       # two models, one frame
                   lambda: mf.cells_global_compensate_bgr_device(None, t, models[0], 1, out=t))                # in place
            for k, call in enumerate(bad):
                assert _status(bbme, call) == -1, k
            raw = [cells(ctx, None, t.data_ptr(), 3 * w - 1, 0, 1, m, 1, 0, None, narrow.data_ptr(), 3 * w, 0, None, None),   # colour pitch
                   cells(ctx, None, t.data_ptr(), 3 * w, 0, 1, m, 1, 0, None, narrow.data_ptr(), 3 * w - 1, 0, None, None),   # output pitch
                   cells(ctx, None, run.data_ptr(), 3 * w, 3 * w * h - 1, 2, models.ctypes.data, 1, 0, None, narrow.data_ptr(), 3 * w,
                         3 * w * h, None, None),                                                                # input stride
                   cells(ctx, None, run.data_ptr(), 3 * w, 3 * w * h, 2, models.ctypes.data, 1, 0, None, narrow.data_ptr(), 3 * w,
                         3 * w * h - 1, None, None),                                                            # output stride
                   cells(ctx, None, t.data_ptr(), 3 * w, 0, 0, m, 1, 0, None, narrow.data_ptr(), 3 * w, 0, None, None),       # no frame
                   cells(ctx, None, t.data_ptr(), 3 * w, 3 * w * h, 33, m, 1, 0, None, narrow.data_ptr(), 3 * w, 3 * w * h, None, None),
                   lib.bbme_global_compensate_bgr_device(ctx, 0, 0, m, 1, 0, t.data_ptr(), 3 * w - 1, None),
                   lib.bbme_global_compensate_bgr_device(ctx, 1, 0, m, 1, 0, t.data_ptr(), 3 * w, None),
                   lib.bbme_global_compensate_bgr_device(ctx, 0, 0, m, 1, 0, None, 3 * w, None)]
            assert raw == [-1] * len(raw), raw
            # a grey setter withdraws the colour
            mf.set_frames(np.ascontiguousarray(a[:, :, 0]), np.ascontiguousarray(b[:, :, 0]))
            assert _status(bbme, lambda: mf.draw_MVimage_global_bgr(models[0])) == -7
            assert _status(bbme, lambda: mf.compensation_error_global_bgr(models[0])) == -7
            assert mf.draw_MVimage_global(models[0]).shape == (mf.padded_height, mf.padded_width)      # the grey call still answers
        mf.close()
    for ctx in (bbme.MFBatch(pairs, search, block), bbme.MFChain(video, search, block)):
        ctx.estimate_bidirectional_async()
        cells = [ctx.get_pair_cells(p) for p in range(3)]
        assert ctx.compensation_errors_global_bgr(models, 1, "forward", window) == single
        assert ctx.compensation_errors_global_bgr(models, 1, "backward", window) == [host[p, "backward"][1] for p in range(3)]
        for p in (2, 0, 1):
            for which in ("forward", "backward"):
                assert np.array_equal(ctx.get_pair_global_compensated_bgr(p, models[p], 1, which, 5), host[p, which][0]), (p, which)
        assert all(np.array_equal(ctx.get_pair_cells(p), cells[p]) for p in range(3))
        ctx.set_direction(True)                                # (a new direction drops the estimate, as it always does)
        assert ctx.compensation_errors_global_bgr(models, 1, "forward", window) == [host[p, "backward"][1] for p in range(3)]
        ctx.close()


# ---- guard bands -------------------------------------------------------------------------------------------------------------
def _guarded_results(bbme):
    """Warps under the edge-straddling model on a single, a batched and a chain context and on a caller's run of frames -> sha256;
    every frame is also held against the host rule"""
    geometry = GEOMETRIES[0]
    w, h, search, block = geometry
    search, block = list(search), list(block)
    px, py = SHAPES[geometry][2:]
    video = _frames(w, h, 3, seed=9)
    model, unit = EDGE_MODEL
    models = np.array([model, tuple(-v for v in model)], np.int32)
    results = []
    ctxs = [bbme.MF(video[0], video[1], search, block), bbme.MFBatch([(video[0], video[1]), (video[1], video[2])], search, block),
            bbme.MFChain(video, search, block)]
    for ctx in ctxs:
        pairs = getattr(ctx, "batch", 1)
        for p in range(pairs):
            got = ctx._get_global_compensated_bgr(p, "forward", models[p], unit, 7, None, "guard")
            exp = bbme.global_compensate_bgr(video[p], video[p + 1], models[p], unit, 7, px, py)
            assert np.array_equal(got, exp[0]), p
            results.append(got)
        st = ctx._global_compensation_stats_bgr("forward", models[:pairs], unit, None)
        assert st == [bbme.global_compensate_bgr(video[p], video[p + 1], models[p], unit, 7, px, py)[1] for p in range(pairs)]
        results.append(np.array([[s[k] for k in STAT_KEYS] for s in st], np.int64))
    got, st = _warp(ctxs[0], video[:2], video[1:], models, unit, 7, (1, 1, w - 3, h - 2), in_extra=1, out_extra=5, out_offset=3)
    for k in range(2):
        exp = bbme.global_compensate_bgr(video[k], video[k + 1], models[k], unit, 7, px, py, (1, 1, w - 3, h - 2))
        assert np.array_equal(got[k], exp[0]) and st[k] == tuple(exp[1][s] for s in STAT_KEYS)
    results += [got, np.array(st, np.int64)]
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
    _capi.check(_capi.lib().bbme_test_guard_find(b"the colour global compensation statistics", 1, C.byref(found)))
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
    for ctx in ctxs:
        ctx.close()
    after = C.c_ulonglong()
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(after), first, len(first)))
    print("GUARDED %s buffer=%d violations=%d after_close=%d %s" % (digest, bool(found.value), violations.value, after.value,
                                                                     first.value.decode()))


def test_guard_bands_and_poison(bbme):
    """The colour store, the statistics scratch and the model tables come from the context's allocation path: between guard bands
    and poisoned, the warps under the edge-straddling model damage no band and give the host rule's frames -- no read of
    unwritten bytes decides a pixel, no write goes outside `out`."""
    ctxs, digest = _guarded_results(bbme)
    for ctx in ctxs:
        ctx.close()
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBME_TEST_GUARD="1", BBME_TEST_POISON="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_global_compensation_bgr as t; t._guard_child()" % (tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:5] == [digest, "buffer=1", "violations=0", "after_close=0"], line[0]


# ---- stabilisation -------------------------------------------------------------------------------------------------------------
def _jitter_video_bgr(w, h, offsets):
    """Frames cut at `offsets` from three independent textures, one per channel (test_gpu_global_motion._jitter_video's recipe)"""
    def texture(seed):
        rng = np.random.default_rng(seed)
        big = rng.integers(0, 256, size=(h + 32, w + 32)).astype(np.float64)
        for _ in range(2):
            big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) / 4
        return np.clip((big - big.mean()) * 3 + 128, 0, 255).astype(np.uint8)
    big = np.stack([texture(seed) for seed in (12, 13, 14)], -1)
    return [np.ascontiguousarray(big[16 + oy:16 + oy + h, 16 + ox:16 + ox + w]) for ox, oy in offsets]


def test_stabilize_frames_on_a_colour_video(bbme):
    from blockbasedmotionestimation_amd import sequence
    w, h, search, block = 96, 64, [16, 16], [8, 8]
    offsets = [(0, 0), (2, -1), (-1, 2), (3, 1), (1, -2)]
    video = _jitter_video_bgr(w, h, offsets)
    grey = [bbme.bgr_to_gray(v) for v in video]
    frames, models, corrections = sequence.stabilize_frames(video, search, block, radius=None, kind="translation")
    _, gmodels, gcorrections = sequence.stabilize_frames(grey, search, block, radius=None, kind="translation")
    assert len(frames) == 5 and models.shape == (4, 6) and corrections.shape == (5, 6)
    assert np.array_equal(models, gmodels) and np.array_equal(corrections, gcorrections)
    exp = np.array([[offsets[f][0] - offsets[f + 1][0], offsets[f][1] - offsets[f + 1][1]] for f in range(4)])
    assert np.array_equal(np.rint(models[:, [0, 3]] / 65536.0).astype(int), exp), models
    m = 8                                                                             # the interior: the jitter stays below it
    for f in range(5):
        assert frames[f].shape == (h, w, 3) and frames[f].dtype == np.uint8
        assert np.array_equal(frames[f][m:h - m, m:w - m], video[0][m:h - m, m:w - m]), f
    # runs shorter than the video (in_flight * batch = 2) give the same frames
    again, _, _ = sequence.stabilize_frames(video, search, block, radius=None, kind="translation", in_flight=2, batch=1)
    assert all(np.array_equal(a, b) for a, b in zip(again, frames))
    frames, models2, corrections = sequence.stabilize_frames(video, search, block, radius=1, kind="translation", fill=3)
    _, _, gcorrections = sequence.stabilize_frames(grey, search, block, radius=1, kind="translation", fill=3)
    assert np.array_equal(models2, models) and np.array_equal(corrections, gcorrections)
    mf = bbme.MF(video[0], video[0], search, block)
    px, py = mf.padding_x, mf.padding_y
    mf.close()
    for f in range(5):
        exp = bbme.global_compensate_bgr(None, video[f], corrections[f], 1, 3, px, py)[0]
        assert np.array_equal(frames[f], exp), f


# ---- the command-line tool -------------------------------------------------------------------------------------------------------
def _write_ppm(path, bgr):
    h, w = bgr.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(bgr[..., ::-1]).tobytes())


def test_cli_writes_the_colour_prediction(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    w, h = 96, 72
    c1, c2 = _jitter_video_bgr(w, h, [(0, 0), (2, -1)])
    _write_ppm(tmp_path / "f1.ppm", c1)
    _write_ppm(tmp_path / "f2.ppm", c2)
    base = [_build.CLI, str(tmp_path / "f1.ppm"), str(tmp_path / "f2.ppm"), "--levels", "2", "--block", "8", "--search", "16"]
    r = subprocess.run(base + ["--no-upsample", "--global-motion", "--gm-out", str(tmp_path / "gm.pgm"), "--gm-out-bgr",
                               str(tmp_path / "gm.ppm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(c1, c2, [16, 16], [8, 8])
    mf.calcMotionBlockMatching()
    g = mf.global_motion()
    frame = mf.draw_MVimage_global_bgr(g["model"])
    assert (tmp_path / "gm.ppm").read_bytes() == b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(frame[..., ::-1]).tobytes()
    grey = mf.draw_MVimage_global(g["model"])
    px, py = mf.padding_x, mf.padding_y
    assert (tmp_path / "gm.pgm").read_bytes() == b"P5\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(grey[py:py + h, px:px + w]).tobytes()
    st = mf.compensation_error_global_bgr(g["model"])
    line = [l for l in r.stdout.splitlines() if l.startswith("Global MC colour PSNR is ")]
    assert len(line) == 1 and line[0] == "Global MC colour PSNR is %.9g dB over %d pixels (%d skipped)" % (st["psnr"], st["pixels"],
                                                                                                         st["skipped"]), r.stdout
    mf.close()
    r = subprocess.run(base + ["--global-motion", "--gm-out-bgr", str(tmp_path / "bad.ppm")], capture_output=True, text=True)
    assert r.returncode == 2 and "--no-upsample" in r.stderr
    r = subprocess.run(base + ["--no-upsample", "--gm-out-bgr", str(tmp_path / "bad.ppm")], capture_output=True, text=True)
    assert r.returncode == 2 and "--global-motion" in r.stderr
