"""K11b k_compensate_bgr against the host rule of the BGR COMPENSATION RULE (bbme_compensate_bgr_host, which
tests/test_compensation_bgr_cpu.py holds against numpy), bit for bit: both units; caller's frames at odd pitches and the stored
colour; every output pitch and the byte path; strided grid rows; the frame alone and the statistics alone; a caller's stream; the
edge and the extreme grids; a full-scale statistics case; B = G = R contexts against the grey calls; single, batched and chain
contexts, `which`, direction BACKWARD and a chain's advance; refusals and state, planes beyond 8188 among them; that unit 1
launches no refinement; the guard bands; sequence.predict_frames on a colour video and on its luma; bbme_cli --mc-subpel.  No
tolerance appears."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import _status
from test_bgr_cpu import SHAPES
from test_compensation_bgr_cpu import frame_windows, grids_for, stats_of
from test_gpu_bidirectional import _oracle_fields
from test_gpu_global_compensation_bgr import _jitter_video_bgr, _write_ppm
from test_subpel_compensation_cpu import FILLS

pytestmark = pytest.mark.gpu

PATTERN = 0x5A
GEOMETRIES = list(SHAPES)                                  # (w, h, search, block) -> pads (1,1), (1,0), (2,2), (0,0)
_cache = {}


def _frames(w, h, count=2, seed=0):
    rng = np.random.default_rng([w, h, seed])
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(count)]


def _cases(bbme, geometry):
    """Per geometry, computed once: the two frames, the pads and per (grid, unit) the fill, the window and the host rule's answer"""
    if geometry not in _cache:
        w, h = geometry[:2]
        px, py = SHAPES[geometry][2:]
        c1, c2 = _frames(w, h)
        windows = frame_windows(w, h)
        cases = []
        for n, (name, grid, unit) in enumerate(grids_for(w, h, px, py)):
            fill, window = FILLS[n % 3], windows[n % len(windows)]
            out, st = bbme.compensate_cells_bgr(c1, c2, grid, unit, fill, px, py, window)
            cases.append((name, grid, unit, fill, window, out, stats_of(st)))
        _cache[geometry] = (c1, c2, px, py, cases)
    return _cache[geometry]


def _pitched(frame, extra):
    """(H, W, 3) view of a buffer whose rows are `extra` bytes further apart than packed; the gaps hold a pattern"""
    import torch
    h, w = frame.shape[:2]
    pitch = 3 * w + extra
    buf = torch.full((pitch * h,), 0xC3, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (h, w, 3), (pitch, 3, 1))
    view.copy_(torch.from_numpy(frame).cuda())
    return view


def _grid_tensor(grid, extra=0):
    """(CH, CW, 2) int16 view whose rows are `extra` cells further apart than packed; the gaps hold far vectors"""
    import torch
    ch, cw = grid.shape[:2]
    buf = torch.full((ch * (cw + extra) * 2,), 0x7A7A, dtype=torch.int16, device="cuda")
    view = torch.as_strided(buf, (ch, cw, 2), (2 * (cw + extra), 2, 1))
    view.copy_(torch.from_numpy(np.ascontiguousarray(grid)).cuda())
    return view


def _compensate(mf, t1, t2, grid, unit, fill=0, window=None, want=("out", "stats"), out_extra=0, out_offset=0, stream=None):
    """cells_compensate_bgr_device -> (frame (H, W, 3) or None, stats tuple or None).  The output lies out_offset bytes into a
    buffer of PATTERN, rows out_extra bytes further apart than packed; nothing outside the frame's pixels may change."""
    import torch
    h, w = mf.orig_height, mf.orig_width
    pitch = 3 * w + out_extra
    whole = torch.full((out_offset + pitch * h + 16,), PATTERN, dtype=torch.uint8, device="cuda") if "out" in want else None
    out = None if whole is None else torch.as_strided(whole, (h, w, 3), (pitch, 3, 1), out_offset)
    st = torch.full((4,), -7, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    mf.cells_compensate_bgr_device(t1 if "stats" in want else None, t2, grid, unit, out, st, fill, window,
                                   None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    got = None
    if whole is not None:
        host = whole.cpu().numpy()
        view = np.lib.stride_tricks.as_strided(host[out_offset:], (h, w, 3), (pitch, 3, 1))
        got = view.copy()
        view[...] = PATTERN
        assert (host == PATTERN).all(), "bytes outside the frame's pixels changed"
    return got, None if st is None else tuple(st.cpu().tolist())


def _context(bbme, geometry, frames=None):
    w, h, search, block = geometry
    c1, c2 = frames if frames is not None else _frames(w, h)
    mf = bbme.MF(c1, c2, list(search), list(block))
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == SHAPES[geometry]
    return mf


# ---- parity with the host rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g[:2])
def test_cells_call_equals_the_host_rule(bbme, geometry):
    """Every grid of grids_for -- fractions, edges, the int16 extremes, far integer cells, zero -- in its unit"""
    c1, c2, px, py, cases = _cases(bbme, geometry)
    mf = _context(bbme, geometry, (c1, c2))
    s1, s2 = mf.frame_bgr_tensor(0, 0), mf.frame_bgr_tensor(0, 1)                      # the context's own, pitch 3 W
    assert np.array_equal(s1.cpu().numpy(), c1) and np.array_equal(s2.cpu().numpy(), c2)
    for n, (name, grid, unit, fill, window, exp_out, exp_st) in enumerate(cases):
        in_extra, kw = (1, 5)[n % 2], dict(out_extra=(0, 1, 5)[n % 3], out_offset=n % 4)
        t1, t2, g = _pitched(c1, in_extra), _pitched(c2, in_extra), _grid_tensor(grid, (0, 3)[n % 2])
        got, st = _compensate(mf, t1, t2, g, unit, fill, window, **kw)
        assert np.array_equal(got, exp_out), (name, unit, kw)
        assert st == exp_st, (name, unit, window)
        got, st = _compensate(mf, s1, s2, _grid_tensor(grid, 1), unit, fill, window, out_extra=kw["out_extra"], out_offset=(n + 1) % 4)
        assert np.array_equal(got, exp_out) and st == exp_st, (name, unit, "stored colour")
        # the frame alone (no frame 1) and the statistics alone
        got, none = _compensate(mf, None, t2, g, unit, fill, None, want=("out",), out_offset=(n + 2) % 4, out_extra=kw["out_extra"])
        assert none is None and np.array_equal(got, exp_out), (name, unit)
        none, st = _compensate(mf, t1, t2, g, unit, 255 - fill, window, want=("stats",))
        assert none is None and st == exp_st, (name, unit)
    mf.close()


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dx%d" % g[:2])
def test_every_output_pitch_and_byte_offset_and_a_callers_stream(bbme, geometry):
    """Output pitches 3 W, 3 W + 1 and 3 W + 5 at base offsets 0..3 under the edge grids of both units: the dword path, the byte
    path and the rows that change between them; every second launch on a caller's stream"""
    import torch
    c1, c2, px, py, cases = _cases(bbme, geometry)
    mf = _context(bbme, geometry)
    stream = torch.cuda.Stream()
    n = 0
    for name, grid, unit, fill, window, exp_out, exp_st in [c for c in cases if c[0] == "edges"]:
        for out_extra in (0, 1, 5):
            for out_offset in (0, 1, 2, 3):
                n += 1
                in_extra = (1, 5)[n % 2]
                got, st = _compensate(mf, _pitched(c1, in_extra), _pitched(c2, in_extra), _grid_tensor(grid, n % 3), unit, fill, window,
                                      out_extra=out_extra, out_offset=out_offset, stream=stream if n % 2 else None)
                assert np.array_equal(got, exp_out) and st == exp_st, (unit, out_extra, out_offset, in_extra)
    mf.close()


def test_full_scale_statistics(bbme):
    """C1 = 0 and C2 = 255 under a zero grid: every lane's sums are the largest they can be; sse = 3 W H 255^2 exactly"""
    import torch
    geometry = min(GEOMETRIES, key=lambda g: g[0] * g[1])
    w, h = geometry[:2]
    mf = _context(bbme, geometry)
    zero = torch.zeros(mf.cells_shape + (2,), dtype=torch.int16, device="cuda")
    t1 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    t2 = torch.full((h, w, 3), 255, dtype=torch.uint8, device="cuda")
    for unit in (1, 4):
        got, st = _compensate(mf, t1, t2, zero, unit, 9)
        assert (got == 255).all()
        assert st == (3 * w * h * 65025, 3 * w * h * 255, w * h, 0), (unit, st)
    mf.close()


def test_planes_beyond_8188_are_refused_and_nothing_is_written(bbme):
    """Frames of 8190 x 130 pad to 8192 x 132: the context's own calls answer ERR_UNSUPPORTED before anything is launched"""
    import torch
    from blockbasedmotionestimation_amd import _capi
    w, h = 8190, 130
    z = np.zeros((h, w, 3), np.uint8)
    mf = bbme.MF(z, z, [12], [4])
    assert (mf.padded_width, mf.padded_height) == (8192, 132)
    out = torch.full((h, w, 3), PATTERN, dtype=torch.uint8, device="cuda")
    host = np.full((h, w, 3), PATTERN, np.uint8)
    calls = (lambda: mf.draw_MVimage_bgr(out=host), lambda: mf.draw_MVimage_subpel_bgr(out=host),
             lambda: mf.compensation_error_bgr(), lambda: mf.compensation_error_subpel_bgr(),
             lambda: _capi.check(mf._lib.bbme_compensate_bgr_device(mf._ctx, 0, 0, 1, 0, out.data_ptr(), 3 * w, None)),
             lambda: _capi.check(mf._lib.bbme_compensate_bgr_device(mf._ctx, 0, 0, 4, 0, out.data_ptr(), 3 * w, None)))
    for k, call in enumerate(calls):
        assert _status(bbme, call) == _capi.ERR_UNSUPPORTED == -8, k
    mf.synchronize()
    torch.cuda.synchronize()
    assert (out == PATTERN).all() and (host == PATTERN).all()
    mf.close()


# ---- B = G = R: the grey calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", GEOMETRIES[:3], ids=lambda g: "%dx%d" % g[:2])
def test_grey_equivalence(bbme, geometry):
    w, h = geometry[:2]
    px, py = SHAPES[geometry][2:]
    g1, g2, _ = bbme.synth_pair(w, h, 17 + w, max_motion=3)
    mf = _context(bbme, geometry, (np.repeat(g1[:, :, None], 3, 2), np.repeat(g2[:, :, None], 3, 2)))
    mf.estimate_bidirectional_async()
    window = (2, 1, w - 7, h - 4)
    pwin = (window[0] + px, window[1] + py) + window[2:]

    def same(colour, grey, cst, gst, what):
        assert colour.shape == (h, w, 3)
        for c in range(3):
            assert np.array_equal(colour[:, :, c], grey[py:py + h, px:px + w]), (what, c)
        assert (cst["sse"], cst["sad"], cst["pixels"], cst["skipped"]) == (3 * gst["sse"], 3 * gst["sad"], gst["pixels"], gst["skipped"]), what
        assert cst["pixels"] > 0 and cst["mse"] == gst["mse"]

    same(mf.draw_MVimage_bgr("forward", 9), mf.draw_MVimage(0, 2, 9), mf.compensation_error_bgr("forward", window),
         mf.compensation_error(0, 2, pwin), "integer")
    for which in ("forward", "backward"):
        same(mf.draw_MVimage_subpel_bgr(which, 9), mf.draw_MVimage_subpel(which, 9), mf.compensation_error_subpel_bgr(which, window),
             mf.compensation_error_subpel(which, pwin), which)
    mf.close()


# ---- context forms -------------------------------------------------------------------------------------------------------------
def _expected(bbme, ctx, p, which, unit, a, b, fill, window):
    """The host rule on the context's own cells of pair p: (frame, statistics dict)"""
    px, py = ctx.padding_x, ctx.padding_y
    batch = hasattr(ctx, "batch")
    if unit == 4:
        grid = ctx.get_pair_subpel_cells(p, which) if batch else ctx.subpel_cells(which)
    elif which == "backward":
        grid = ctx.get_pair_backward_cells(p) if batch else ctx.get_backward_cells()
    else:
        grid = ctx.get_pair_cells(p) if batch else ctx.get_cells()
    c1, c2 = (a, b) if which == "forward" else (b, a)
    return bbme.compensate_cells_bgr(c1, c2, grid, unit, fill, px, py, window)


def test_context_forms_direction_state_and_refusals(bbme):
    import torch
    geometry = GEOMETRIES[0]
    w, h, search, block = geometry
    search, block = list(search), list(block)
    video = _jitter_video_bgr(w, h, [(0, 0), (2, -1), (-1, 2), (3, 1), (1, -2), (0, 2)])
    pairs = [(video[p], video[p + 1]) for p in range(3)]
    window = (1, 0, w - 3, h - 1)
    single = {}
    for p, (a, b) in enumerate(pairs):
        mf = bbme.MF(a, b, search, block)
        mf.estimate_bidirectional_async()
        before = [mf.get_cells(), mf.get_flow(), mf.get_backward_cells()]
        for which in ("forward", "backward"):
            for unit, draw, error in ((1, mf.draw_MVimage_bgr, mf.compensation_error_bgr),
                                      (4, mf.draw_MVimage_subpel_bgr, mf.compensation_error_subpel_bgr)):
                exp_out, _ = _expected(bbme, mf, 0, which, unit, a, b, 5, None)
                _, exp_st = _expected(bbme, mf, 0, which, unit, a, b, 5, window)
                assert np.array_equal(draw(which, 5), exp_out), (p, which, unit)
                single[p, which, unit] = error(which, window)
                assert single[p, which, unit] == exp_st, (p, which, unit)
        after = [mf.get_cells(), mf.get_flow(), mf.get_backward_cells()]
        assert all(np.array_equal(x, y) for x, y in zip(before, after))                # no state changed ...
        mf.calcMotionBlockMatching()
        assert np.array_equal(mf.get_cells(), before[0])                               # ... and a later estimate is the same
        if p == 0:
            # direction BACKWARD exchanges the frames (a new direction drops the estimate, as it always does)
            mf.set_direction(True)
            mf.calcMotionBlockMatching()
            for unit, draw, error in ((1, mf.draw_MVimage_bgr, mf.compensation_error_bgr),
                                      (4, mf.draw_MVimage_subpel_bgr, mf.compensation_error_subpel_bgr)):
                exp_out, exp_st = _expected(bbme, mf, 0, "forward", unit, b, a, 5, None)
                assert np.array_equal(draw("forward", 5), exp_out) and error("forward") == exp_st, unit
            mf.set_direction(False)
            mf.calcMotionBlockMatching()
            # refusals
            t = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            narrow = torch.zeros((h, 3 * w - 1), dtype=torch.uint8, device="cuda")
            g = torch.zeros(mf.cells_shape + (2,), dtype=torch.int16, device="cuda")
            st = torch.zeros(4, dtype=torch.int64, device="cuda")
            bad = (lambda: mf.draw_MVimage_bgr("forward", 256), lambda: mf.draw_MVimage_subpel_bgr(2),
                   lambda: mf.compensation_error_bgr("forward", (0, 0, w + 1, 2)),
                   lambda: mf.compensation_error_subpel_bgr("forward", (0, 0, w, 0)),
                   lambda: mf.cells_compensate_bgr_device(None, t, g, 4),                                  # neither out nor stats
                   lambda: mf.cells_compensate_bgr_device(None, t, g, 4, stats=st),                        # stats without frame 1
                   lambda: mf.cells_compensate_bgr_device(None, t, g, 2, out=t.clone()),                   # unit
                   lambda: mf.cells_compensate_bgr_device(None, t, g[:, :-1], 4, out=t.clone()),           # a narrower grid
                   lambda: mf.cells_compensate_bgr_device(None, t, g, 4, out=t))                           # in place
            for k, call in enumerate(bad):
                assert _status(bbme, call) == -1, k
            lib, ctx = mf._lib, mf._ctx
            cells, cw = lib.bbme_cells_compensate_bgr_device, mf.cells_shape[1]
            raw = [cells(ctx, None, t.data_ptr(), 3 * w - 1, g.data_ptr(), cw, 4, 0, None, narrow.data_ptr(), 3 * w, None, None),      # colour pitch
                   cells(ctx, None, t.data_ptr(), 3 * w, g.data_ptr(), cw, 4, 0, None, narrow.data_ptr(), 3 * w - 1, None, None),      # output pitch
                   cells(ctx, None, t.data_ptr(), 3 * w, g.data_ptr(), cw - 1, 4, 0, None, narrow.data_ptr(), 3 * w, None, None),      # grid pitch
                   cells(ctx, None, t.data_ptr(), 3 * w, None, cw, 4, 0, None, narrow.data_ptr(), 3 * w, None, None),                  # no grid
                   lib.bbme_compensate_bgr_device(ctx, 0, 0, 4, 0, t.data_ptr(), 3 * w - 1, None),
                   lib.bbme_compensate_bgr_device(ctx, 1, 0, 4, 0, t.data_ptr(), 3 * w, None),
                   lib.bbme_compensate_bgr_device(ctx, 0, 0, 3, 0, t.data_ptr(), 3 * w, None),
                   lib.bbme_compensate_bgr_device(ctx, 0, 0, 4, 0, None, 3 * w, None),
                   lib.bbme_get_compensated_bgr_host(ctx, 0, 0, 4, 0, None),
                   lib.bbme_compensation_error_bgr(ctx, 0, 4, None, None)]
            assert raw == [-1] * len(raw), raw
            # a grey setter withdraws the colour
            mf.set_frames(np.ascontiguousarray(a[:, :, 0]), np.ascontiguousarray(b[:, :, 0]))
            mf.calcMotionBlockMatching()
            for call in (mf.draw_MVimage_bgr, mf.draw_MVimage_subpel_bgr, mf.compensation_error_bgr, mf.compensation_error_subpel_bgr):
                assert _status(bbme, call) == -7
            assert mf.draw_MVimage_subpel().shape == (mf.padded_height, mf.padded_width)       # the grey call still answers
        mf.close()
    for ctx in (bbme.MFBatch(pairs, search, block), bbme.MFChain(video[:4], search, block)):
        ctx.estimate_bidirectional_async()
        cells = [ctx.get_pair_cells(p) for p in range(3)]
        for which in ("forward", "backward"):
            for unit in (1, 4):
                every = ctx.compensation_errors_bgr(unit, which, window)
                assert every == [single[p, which, unit] for p in range(3)], (which, unit)
                for p in (2, 0, 1):
                    exp_out, _ = _expected(bbme, ctx, p, which, unit, pairs[p][0], pairs[p][1], 5, None)
                    assert np.array_equal(ctx.get_pair_motion_compensated_bgr(p, unit, which, 5), exp_out), (p, which, unit)
        assert all(np.array_equal(ctx.get_pair_cells(p), cells[p]) for p in range(3))
        if isinstance(ctx, bbme.MFChain):
            # after the roll: slot 3 became slot 0, two new frames and a repeat behind it
            ctx.advance([video[4], video[5], video[5]])
            ctx.estimate_async()
            rolled = [(video[3], video[4]), (video[4], video[5])]
            for unit in (1, 4):
                every = ctx.compensation_errors_bgr(unit, "forward", window)
                for p, (a, b) in enumerate(rolled):
                    exp_out, _ = _expected(bbme, ctx, p, "forward", unit, a, b, 5, None)
                    _, exp_st = _expected(bbme, ctx, p, "forward", unit, a, b, 5, window)
                    assert np.array_equal(ctx.get_pair_motion_compensated_bgr(p, unit, "forward", 5), exp_out), (p, unit)
                    assert every[p] == exp_st, (p, unit)
        ctx.close()


# ---- guard bands, and the quarter-pel buffer under unit 1 ---------------------------------------------------------------------
def _guarded_results(bbme):
    """Predictions in both units on a single, a batched and a chain context and on a caller's frames under the edge grid ->
    sha256; every frame is also held against the host rule"""
    geometry = GEOMETRIES[0]
    w, h, search, block = geometry
    search, block = list(search), list(block)
    px, py = SHAPES[geometry][2:]
    video = _jitter_video_bgr(w, h, [(0, 0), (2, -1), (-1, 2)])
    results = []
    ctxs = [bbme.MF(video[0], video[1], search, block), bbme.MFBatch([(video[0], video[1]), (video[1], video[2])], search, block),
            bbme.MFChain(video, search, block)]
    for ctx in ctxs:
        ctx.estimate_async()
        pairs = getattr(ctx, "batch", 1)
        for unit in (1, 4):
            st = ctx._compensation_stats_bgr("forward", unit, None)
            for p in range(pairs):
                got = ctx._get_compensated_bgr(p, "forward", unit, 7, None, "guard")
                grid = (ctx._subpel_cells(p, "forward", None, "guard") if unit == 4 else
                        ctx.get_pair_cells(p) if hasattr(ctx, "batch") else ctx.get_cells())
                exp = bbme.compensate_cells_bgr(video[p], video[p + 1], grid, unit, 7, px, py)
                assert np.array_equal(got, exp[0]) and st[p] == exp[1], (p, unit)
                results.append(got)
            results.append(np.array([stats_of(s) for s in st], np.int64))
    c1, c2, _, _, cases = _cases(bbme, geometry)
    for name, grid, unit, fill, window, exp_out, exp_st in [c for c in cases if c[0] in ("edges", "extremes")]:
        got, st = _compensate(ctxs[0], _pitched(c1, 1), _pitched(c2, 1), _grid_tensor(grid, 3), unit, fill, window, out_extra=5,
                              out_offset=3)
        assert np.array_equal(got, exp_out) and st == exp_st, (name, unit)
        results += [got, np.array(st, np.int64)]
    return ctxs, hashlib.sha256(b"".join(np.ascontiguousarray(r).tobytes() for r in results)).hexdigest()


def _unit_1_leaves_the_quarter_pel_buffer(bbme):
    """Under BBME_TEST_GUARD: a context that has only predicted along integer cells has no quarter-pel buffer at all; once unit 4
    has made it, unit 1 calls on NEW frames -- whose refinement would give other vectors -- leave every byte of it as it was."""
    import ctypes as C
    import torch
    from blockbasedmotionestimation_amd import _capi
    geometry = GEOMETRIES[0]
    w, h, search, block = geometry
    video = _jitter_video_bgr(w, h, [(0, 0), (2, -1), (-1, 2)])
    mf = bbme.MF(video[0], video[1], list(search), list(block))
    mf.estimate_async()
    what, found = b"the quarter-pel cells of the compensation", C.c_void_p()
    mf.draw_MVimage_bgr()
    mf.compensation_error_bgr()
    assert _capi.lib().bbme_test_guard_find(what, 0, C.byref(found)) == _capi.ERR_INVALID      # never allocated
    mf.draw_MVimage_subpel_bgr()
    _capi.check(_capi.lib().bbme_test_guard_find(what, 0, C.byref(found)))
    ch, cw = mf.cells_shape
    q4 = mf._hbm_view(found.value + 4096, (ch, cw, 2), "<i2")                              # the payload behind the front band
    assert np.array_equal(q4.cpu().numpy(), mf.subpel_cells())
    kept = q4.clone()
    mf.set_frames(video[1], video[2])
    mf.estimate_async()
    assert not np.array_equal(mf.subpel_cells(), kept.cpu().numpy())                       # a refinement would change it
    mf.draw_MVimage_bgr()
    mf.compensation_error_bgr()
    mf.synchronize()
    torch.cuda.synchronize()
    unchanged = bool((q4 == kept).all())
    mf.draw_MVimage_subpel_bgr()
    refined = np.array_equal(q4.cpu().numpy(), mf.subpel_cells())
    mf.close()
    return unchanged and refined


def _guard_child():
    """Runs in a fresh process under BBME_TEST_GUARD=1 and BBME_TEST_POISON=1: prints the digest of the results and the guards' state"""
    import ctypes as C
    import blockbasedmotionestimation_amd as bbme
    from blockbasedmotionestimation_amd import _capi
    assert os.environ["BBME_TEST_GUARD"] == "1" and os.environ["BBME_TEST_POISON"] == "1"
    q4_kept = _unit_1_leaves_the_quarter_pel_buffer(bbme)
    ctxs, digest = _guarded_results(bbme)
    live, violations, first = C.c_ulonglong(), C.c_ulonglong(), C.create_string_buffer(512)
    found = C.c_void_p()
    _capi.check(_capi.lib().bbme_test_guard_find(b"the colour compensation statistics", 1, C.byref(found)))
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
    for ctx in ctxs:
        ctx.close()
    after = C.c_ulonglong()
    _capi.check(_capi.lib().bbme_test_guard_check(C.byref(live), C.byref(after), first, len(first)))
    print("GUARDED %s buffer=%d violations=%d after_close=%d q4_kept=%d %s" % (digest, bool(found.value), violations.value, after.value,
                                                                               q4_kept, first.value.decode()))


def test_guard_bands_poison_and_no_refinement_under_unit_1(bbme):
    """The colour store, the statistics scratch and the quarter-pel buffer come from the context's allocation path: between guard
    bands and poisoned, the predictions damage no band and give the host rule's frames -- no read of unwritten bytes decides a
    pixel, no write goes outside `out` --, and unit 1 neither makes nor touches the quarter-pel buffer."""
    ctxs, digest = _guarded_results(bbme)
    for ctx in ctxs:
        ctx.close()
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BBME_TEST_GUARD="1", BBME_TEST_POISON="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_compensation_bgr as t; t._guard_child()" % (tests, os.path.dirname(tests))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("GUARDED ")]
    assert len(line) == 1, r.stdout + r.stderr
    assert line[0].split()[1:6] == [digest, "buffer=1", "violations=0", "after_close=0", "q4_kept=1"], line[0]


# ---- the video driver ------------------------------------------------------------------------------------------------------------
def test_predict_frames_on_a_colour_video_and_on_its_luma(bbme, oracle):
    from blockbasedmotionestimation_amd import sequence
    w, h, search, block = 132, 100, [16, 16], [8, 8]
    video = _jitter_video_bgr(w, h, [(0, 0), (2, -1), (-1, 2), (3, 1), (1, -2)])
    grey = [bbme.bgr_to_gray(v) for v in video]
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    fields = []
    for k in range(4):
        _, cells = _oracle_fields(bbme, oracle, grey[k], grey[k + 1], search, block)
        p1, p2 = bbme.pad_zero(grey[k], px, py), bbme.pad_zero(grey[k + 1], px, py)
        fields.append((cells, bbme.subpel_cells(p1, p2, cells)[0], p1, p2))
    for subpel in (True, False):
        frames, stats = sequence.predict_frames(video, search, block, subpel=subpel)
        gframes, gstats = sequence.predict_frames(grey, search, block, subpel=subpel, in_flight=2, batch=1)
        assert len(frames) == len(gframes) == 4 and stats.shape == gstats.shape == (4, 4)
        for k, (cells, q4, p1, p2) in enumerate(fields):
            exp, st = bbme.compensate_cells_bgr(video[k], video[k + 1], q4 if subpel else cells, 4 if subpel else 1, 0, px, py)
            assert frames[k].shape == (h, w, 3) and np.array_equal(frames[k], exp), (subpel, k)
            assert tuple(int(v) for v in stats[k]) == stats_of(st), (subpel, k)
            gexp, gst = bbme.compensate_cells_subpel(p1, p2, q4 if subpel else (4 * cells).astype(np.int16), 0, (px, py, w, h))
            assert gframes[k].shape == (h, w) and np.array_equal(gframes[k], gexp[py:py + h, px:px + w]), (subpel, k)
            assert tuple(int(v) for v in gstats[k]) == stats_of(gst), (subpel, k)
    assert sequence.predict_frames(video[:1], search, block)[1].shape == (0, 4)


# ---- the command-line tool -------------------------------------------------------------------------------------------------------
def test_cli_writes_the_colour_predictions(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    w, h = 96, 72
    c1, c2 = _jitter_video_bgr(w, h, [(0, 0), (2, -1)])
    _write_ppm(tmp_path / "f1.ppm", c1)
    _write_ppm(tmp_path / "f2.ppm", c2)
    base = [_build.CLI, str(tmp_path / "f1.ppm"), str(tmp_path / "f2.ppm"), "--levels", "2", "--block", "8", "--search", "16"]
    r = subprocess.run(base + ["--no-upsample", "--mc", str(tmp_path / "mc.pgm"), "--mc-subpel", str(tmp_path / "mcq.pgm")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(c1, c2, [16, 16], [8, 8])
    mf.calcMotionBlockMatching()
    px, py = mf.padding_x, mf.padding_y
    ppm = lambda f: b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(f[..., ::-1]).tobytes()      # noqa: E731
    pgm = lambda f: b"P5\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(f[py:py + h, px:px + w]).tobytes()      # noqa: E731
    assert (tmp_path / "mcq.ppm").read_bytes() == ppm(mf.draw_MVimage_subpel_bgr())
    assert (tmp_path / "mc.ppm").read_bytes() == ppm(mf.draw_MVimage_bgr())
    assert (tmp_path / "mcq.pgm").read_bytes() == pgm(mf.draw_MVimage_subpel())
    assert (tmp_path / "mc.pgm").read_bytes() == pgm(mf.draw_MVimage(0, 2))
    s1, s4 = mf.compensation_error_bgr(), mf.compensation_error_subpel_bgr()
    lines = r.stdout.splitlines()
    assert "MC colour PSNR is %.9g dB over %d pixels (%d skipped)" % (s1["psnr"], s1["pixels"], s1["skipped"]) in lines, r.stdout
    assert ("Quarter-pel MC colour PSNR is %.9g dB (integer vectors: %.9g dB) over %d pixels (%d skipped)"
            % (s4["psnr"], s1["psnr"], s4["pixels"], s4["skipped"])) in lines, r.stdout
    mf.close()
    # grey frames and up-sampled colour frames write no colour file
    r = subprocess.run(base + ["--mc-subpel", str(tmp_path / "up.pgm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and (tmp_path / "up.pgm").exists() and not (tmp_path / "up.ppm").exists()
