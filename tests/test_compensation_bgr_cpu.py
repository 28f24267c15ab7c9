"""The BGR compensation rule of include/bbme.h on the CPU: bbme_compensate_bgr_host against a numpy restatement written here --
the subpel compensation rule's restatement on each channel of the zero-padded view, cropped --, the rule's properties against
the existing grey host calls, its refusals, and integer against quarter-pel colour prediction on the Venus-warped pair.  No GPU.
Everything is bit for bit; no tolerance appears."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_bgr_cpu import SHAPES, np_bgr_to_gray
from test_subpel_compensation_cpu import (FILLS, STAT_KEYS, edge_grid, extreme_grid, fraction_grid, np_subpel_compensate,
                                          odd_windows)

NEW_SYMBOLS = ["bbme_compensate_bgr_host", "bbme_cells_compensate_bgr_device", "bbme_compensate_bgr_device",
               "bbme_get_compensated_bgr_host", "bbme_compensation_error_bgr"]

GEOMETRIES = [(w, h, px, py) for (w, h, _, _), (_, _, px, py) in SHAPES.items()]      # pads (1,1), (1,0), (2,2), (0,0)
PITCH_EXTRA = (0, 1, 5)


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def np_compensate_bgr(c1, c2, grid, unit, fill=0, pad_x=0, pad_y=0, window=None):
    """The rule in its own words: the subpel compensation rule on every channel of the zero-padded view along 4 / unit times
    the grid (in 64 bits), the unpadded crop of it; statistics over the window moved into the padded view, sse and sad added
    over the channels."""
    c2 = np.asarray(c2, np.uint8)
    h, w = c2.shape[:2]
    q = np.asarray(grid).astype(np.int64) * (4 // unit)
    win = (0, 0, w, h) if window is None else window
    pwin = (win[0] + pad_x, win[1] + pad_y, win[2], win[3])
    out = np.empty((h, w, 3), np.uint8)
    stats = None
    for c in range(3):
        p2 = np.pad(c2[:, :, c], ((pad_y, pad_y), (pad_x, pad_x)))
        p1 = None if c1 is None else np.pad(np.asarray(c1, np.uint8)[:, :, c], ((pad_y, pad_y), (pad_x, pad_x)))
        o, st = np_subpel_compensate(p1, p2, q, fill, pwin)
        out[:, :, c] = o[pad_y:pad_y + h, pad_x:pad_x + w]
        if st is not None:
            stats = st if stats is None else (stats[0] + st[0], stats[1] + st[1], stats[2], stats[3])
            assert stats[2:] == st[2:]                                    # pixels and skipped do not depend on the channel
    return out, stats


# ---- the cases (the GPU tests use the same) ------------------------------------------------------------------------------------
def grids_for(w, h, px, py):
    """(name, grid, unit) over the cells of the padded view: every fraction pair, every edge of the padded plane, the int16
    extremes (where 4 G overflows int16 with unit 1), each in both units, and a zero grid."""
    W0, H0 = w + 2 * px, h + 2 * py
    out = []
    for unit in (4, 1):
        out.append(("fractions", fraction_grid(W0, H0, 1 + unit), unit))
        out.append(("edges", edge_grid(W0, H0, 11 + unit)[0], unit))
        out.append(("extremes", extreme_grid(W0, H0, 5 + unit), unit))
    out.append(("far", (fraction_grid(W0, H0, 2, reach=W0 // 8).astype(np.int64) // 4).astype(np.int16), 1))
    out.append(("zero", np.zeros((H0 // 2, W0 // 2, 2), np.int16), 4))
    return out


def frame_windows(w, h):
    return (None,) + odd_windows(w, h)


def pitched(rng, h, w, pitch):
    """A random (h, w, 3) colour frame in a buffer of exactly pitch (h - 1) + 3 w bytes, the gaps random too."""
    buf = rng.integers(0, 256, size=pitch * (h - 1) + 3 * w, dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(buf, (h, w, 3), (pitch, 3, 1))


def strided_grid(grid, extra):
    """The grid in rows `extra` cells further apart, in a buffer of exactly that size, the gaps poisoned."""
    ch, cw = grid.shape[:2]
    buf = np.full(((cw + extra) * (ch - 1) + cw) * 2, 0x7A7A, np.int16)
    view = np.lib.stride_tricks.as_strided(buf, (ch, cw, 2), (4 * (cw + extra), 4, 2))
    view[...] = grid
    return view


def host_rule(c1, c2, w, h, px, py, grid, unit, fill, window, want_out=True, want_stats=True, out_pitch=None):
    """bbme_compensate_bgr_host itself (not the package's wrapper) -> (rc, out or None, stats tuple or None)."""
    from blockbasedmotionestimation_amd import _capi
    out_pitch = 3 * w if out_pitch is None else out_pitch
    out = np.full((h, out_pitch), 0xA5, np.uint8) if want_out else None
    st = (C.c_ulonglong * 4)(*[0xDEAD] * 4) if want_stats else None
    win = None if window is None else (C.c_int * 4)(*window)
    rc = _capi.lib().bbme_compensate_bgr_host(None if c1 is None else c1.ctypes.data, c2.ctypes.data, w, h, c2.strides[0], px, py,
                                              grid.ctypes.data, grid.strides[0] // 4, unit, fill, win,
                                              None if out is None else out.ctypes.data, out_pitch, st)
    return rc, out, (tuple(st) if st is not None else None)


def stats_of(d):
    return tuple(d[k] for k in STAT_KEYS)


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
        assert "int %s(" % name in header, name
    assert "BGR COMPENSATION RULE" in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_compensate_bgr_device(None, d, d, 12, d, 2, 1, 0, None, d, 12, st, None) == inv
    assert L.bbme_compensate_bgr_device(None, 0, 0, 4, 0, d, 12, None) == inv
    assert L.bbme_get_compensated_bgr_host(None, 0, 0, 1, 0, d) == inv
    assert L.bbme_compensation_error_bgr(None, 0, 4, None, st) == inv
    assert "compensate_cells_bgr" in bbme.__all__ and hasattr(bbme, "compensate_cells_bgr")
    for name in ("draw_MVimage_bgr", "draw_MVimage_subpel_bgr", "compensation_error_bgr", "compensation_error_subpel_bgr",
                 "cells_compensate_bgr_device"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        for name in ("get_pair_motion_compensated_bgr", "compensation_errors_bgr"):
            assert hasattr(cls, name), name
    from blockbasedmotionestimation_amd import sequence
    assert hasattr(sequence, "predict_frames")


@pytest.mark.parametrize("extra", PITCH_EXTRA)
@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_host_rule_equals_numpy(bbme, w, h, px, py, extra):
    rng = np.random.default_rng(1000 * w + 10 * px + extra)
    pitch = 3 * w + extra
    c1, c2 = pitched(rng, h, w, pitch), pitched(rng, h, w, pitch)
    windows = frame_windows(w, h)
    skipped = {}
    n = 0
    for name, grid, unit in grids_for(w, h, px, py):
        g = strided_grid(grid, extra)
        per_fill = []
        for fill in FILLS:
            for window in windows if fill == FILLS[0] else windows[:3]:
                n += 1
                exp_out, exp_st = np_compensate_bgr(c1, c2, grid, unit, fill, px, py, window)
                rc, out, st = host_rule(c1, c2, w, h, px, py, g, unit, fill, window, out_pitch=3 * w + (n % 3))
                assert rc == 0
                assert np.array_equal(out[:, :3 * w].reshape(h, w, 3), exp_out), (name, unit, fill)
                assert np.all(out[:, 3 * w:] == 0xA5)                     # nothing written between the rows
                assert st == exp_st, (name, unit, window)
                if window is None:
                    per_fill.append(st)
                    skipped[name] = st[3]
                    assert st[2] + st[3] == w * h
        assert per_fill == [per_fill[0]] * len(FILLS)                     # independent of fill
        # the frame alone, the statistics alone, and the package's wrapper
        exp_out, exp_st = np_compensate_bgr(c1, c2, grid, unit, 7, px, py, windows[1])
        rc, out1, none = host_rule(None, c2, w, h, px, py, g, unit, 7, None, want_stats=False)
        assert rc == 0 and none is None and np.array_equal(out1.reshape(h, w, 3), exp_out)
        rc, none, st1 = host_rule(c1, c2, w, h, px, py, g, unit, 200, windows[1], want_out=False)
        assert rc == 0 and none is None and st1 == exp_st
        wout, wst = bbme.compensate_cells_bgr(c1, c2, g, unit, 7, px, py, windows[1])
        assert np.array_equal(wout, exp_out) and stats_of(wst) == exp_st
        if exp_st[2]:
            assert wst["mse"] == exp_st[0] / (3 * exp_st[2])
            assert exp_st[0] == 0 or wst["psnr"] == 10.0 * math.log10(255.0 ** 2 * 3 * exp_st[2] / exp_st[0])
    assert skipped["zero"] == 0 and all(skipped[k] > 0 for k in ("fractions", "edges", "extremes", "far"))


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_extremes_overflow_int16_with_unit_1(w, h, px, py):
    """What the unit is for: 4 G of the extreme grid does not fit int16, and wrapped to int16 it would name other cells."""
    grid = extreme_grid(w + 2 * px, h + 2 * py, 5 + 1)
    wide = 4 * grid.astype(np.int64)
    assert (wide > 32767).any() and (wide < -32768).any()
    rng = np.random.default_rng(3)
    c2 = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    right, _ = np_compensate_bgr(None, c2, grid, 1, 9, px, py)
    wrapped, _ = np_compensate_bgr(None, c2, wide.astype(np.int16), 4, 9, px, py)
    assert not np.array_equal(right, wrapped)


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_odd_pads_make_cells_straddle_the_frames_edge(w, h, px, py):
    """With an odd pad the frame's first and last column (row) belong to cells whose other column (row) is padding: only the
    pixel inside is written, and the statistics count pixels of the frame alone."""
    W0, H0 = w + 2 * px, h + 2 * py
    assert W0 % 2 == 0 and H0 % 2 == 0
    rng = np.random.default_rng(w)
    c1, c2 = rng.integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    grid = np.zeros((H0 // 2, W0 // 2, 2), np.int16)
    grid[:, 0] = (-4 * W0, 0)                                             # the first column of cells is skipped
    out, st = np_compensate_bgr(c1, c2, grid, 4, 9, px, py)
    first = 2 - px % 2 if px else 2                                       # its pixels inside the frame: one column with an odd pad
    if px >= 2:
        first = 0                                                         # the whole first cell column is padding
    assert st[3] == first * h and st[2] == (w - first) * h
    assert (out[:, :first] == 9).all() and np.array_equal(out[:, first:], c2[:, first:])


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_grey_frames_give_the_grey_rules_on_the_padded_plane(bbme, w, h, px, py):
    from blockbasedmotionestimation_amd import _capi
    rng = np.random.default_rng(7 * w + px)
    g1, g2 = rng.integers(0, 256, size=(2, h, w)).astype(np.uint8)
    c1, c2 = np.repeat(g1[:, :, None], 3, 2), np.repeat(g2[:, :, None], 3, 2)
    p1, p2 = bbme.pad_zero(g1, px, py), bbme.pad_zero(g2, px, py)
    H0, W0 = p1.shape
    for (name, grid, unit), window in zip(grids_for(w, h, px, py), frame_windows(w, h) * 2):
        out, st = bbme.compensate_cells_bgr(c1, c2, grid, unit, 3, px, py, window)
        pwin = (px, py, w, h) if window is None else (window[0] + px, window[1] + py, window[2], window[3])
        if unit == 4:
            gout, gst = bbme.compensate_cells_subpel(p1, p2, grid, 3, pwin)
            gst = stats_of(gst)
        else:                                                             # the integer compensation rule at level 0, block 2
            gout = np.empty((H0, W0), np.uint8)
            s4 = (C.c_ulonglong * 4)()
            assert _capi.lib().bbme_motion_compensate_host(p1.ctypes.data, p2.ctypes.data, W0, H0, grid.ctypes.data, 2, 2, 3,
                                                           (C.c_int * 4)(*pwin), gout.ctypes.data, s4) == 0
            gst = tuple(s4)
        for c in range(3):
            assert np.array_equal(out[:, :, c], gout[py:py + h, px:px + w]), (name, unit, c)
        assert (st["sse"], st["sad"], st["pixels"], st["skipped"]) == (3 * gst[0], 3 * gst[1], gst[2], gst[3]), (name, unit)


def test_without_padding_each_channel_is_the_grey_rule(bbme):
    rng = np.random.default_rng(11)
    h, w = 50, 70
    c1, c2 = rng.integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    for name, grid, unit in grids_for(w, h, 0, 0):
        if unit != 4:
            continue
        out, st = bbme.compensate_cells_bgr(c1, c2, grid, 4, 9)
        sse = sad = 0
        for c in range(3):
            gout, gst = bbme.compensate_cells_subpel(np.ascontiguousarray(c1[:, :, c]), np.ascontiguousarray(c2[:, :, c]), grid, 9)
            assert np.array_equal(out[:, :, c], gout), (name, c)
            sse, sad = sse + gst["sse"], sad + gst["sad"]
            assert (st["pixels"], st["skipped"]) == (gst["pixels"], gst["skipped"])
        assert (st["sse"], st["sad"]) == (sse, sad)


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_unit_1_is_unit_4_on_four_times_the_grid(bbme, w, h, px, py):
    rng = np.random.default_rng(w + 3 * py)
    c1, c2 = rng.integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    G = rng.integers(-8191, 8192, size=((h + 2 * py) // 2, (w + 2 * px) // 2, 2)).astype(np.int16)
    near = rng.random(G.shape[:2]) < 0.8
    G[near] = rng.integers(-6, 7, size=(int(near.sum()), 2))
    G[0, 0], G[-1, -1] = (-8192, 8191), (8191, -8192)                     # 4 G = -32768 and 32764: the ends of int16
    for window in (None, (1, 1, w - 3, h - 3)):
        a, sa = bbme.compensate_cells_bgr(c1, c2, G, 1, 5, px, py, window)
        b, sb = bbme.compensate_cells_bgr(c1, c2, (4 * G.astype(np.int64)).astype(np.int16), 4, 5, px, py, window)
        assert np.array_equal(a, b) and stats_of(sa) == stats_of(sb)
        assert sa["pixels"] > 0 and sa["skipped"] > 0


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_zero_grid_returns_frame_2(bbme, w, h, px, py):
    rng = np.random.default_rng(w + h + px)
    c1, c2 = rng.integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    zero = np.zeros(((h + 2 * py) // 2, (w + 2 * px) // 2, 2), np.int16)
    d = c2.astype(np.int64) - c1.astype(np.int64)
    for unit in (1, 4):
        out, st = bbme.compensate_cells_bgr(c1, c2, zero, unit, 77, px, py)
        assert np.array_equal(out, c2)
        assert stats_of(st) == (int((d * d).sum()), int(np.abs(d).sum()), w * h, 0)
        x0, y0, ww, hh = 3, 5, 7, 9
        dw = d[y0:y0 + hh, x0:x0 + ww]
        _, st = bbme.compensate_cells_bgr(c1, c2, zero, unit, 77, px, py, (x0, y0, ww, hh))
        assert stats_of(st) == (int((dw * dw).sum()), int(np.abs(dw).sum()), ww * hh, 0)


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    f = _capi.lib().bbme_compensate_bgr_host
    w, h = 20, 16
    cw = (w + 2) // 2
    c = np.zeros((h, w, 3), np.uint8)
    out = np.zeros((h, w, 3), np.uint8)
    grid = np.zeros(((h + 2) // 2, cw, 2), np.int16)
    st = (C.c_ulonglong * 4)()
    win = lambda *v: (C.c_int * 4)(*v)                                    # noqa: E731
    p, o, g = c.ctypes.data, out.ctypes.data, grid.ctypes.data
    bad = [
        f(p, None, w, h, 3 * w, 1, 1, g, cw, 1, 0, None, o, 3 * w, st),       # no frame 2
        f(p, p, w, h, 3 * w, 1, 1, None, cw, 1, 0, None, o, 3 * w, st),       # no grid
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 1, 0, None, None, 3 * w, None),     # neither out nor statistics
        f(None, p, w, h, 3 * w, 1, 1, g, cw, 1, 0, None, None, 3 * w, st),    # statistics without frame 1
        f(p, p, 0, h, 3 * w, 1, 1, g, cw, 1, 0, None, o, 3 * w, st),
        f(p, p, w, h, 3 * w, -1, 1, g, cw, 1, 0, None, o, 3 * w, st),
        f(p, p, w - 1, h, 3 * w, 1, 1, g, cw, 1, 0, None, o, 3 * w, st),      # the padded view is odd
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 2, 0, None, o, 3 * w, st),          # unit
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 0, 0, None, o, 3 * w, st),
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 256, None, o, 3 * w, st),        # fill
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, -1, None, o, 3 * w, st),
        f(p, p, w, h, 3 * w - 1, 1, 1, g, cw, 4, 0, None, o, 3 * w, st),      # colour pitch
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 0, None, o, 3 * w - 1, st),      # output pitch
        f(p, p, w, h, 3 * w, 1, 1, g, cw - 1, 4, 0, None, o, 3 * w, st),      # grid pitch
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 0, win(0, 0, w + 1, 1), o, 3 * w, st),      # the window is in FRAME pixels
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 0, win(-1, 0, 2, 1), o, 3 * w, st),
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 0, win(0, 0, 0, 1), o, 3 * w, st),
        f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 0, win(0, h - 1, 1, 2), o, 3 * w, st),
    ]
    assert bad == [_capi.ERR_INVALID] * len(bad), bad
    assert f(None, p, w, h, 3 * w, 1, 1, g, cw, 1, 0, None, o, 3 * w, None) == 0      # frame 1 may be null without statistics
    assert f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 0, None, None, 0, st) == 0            # out may be null with statistics
    assert f(p, p, w, h, 3 * w, 1, 1, g, cw, 4, 255, win(w - 1, h - 1, 1, 1), o, 3 * w, st) == 0
    for args in ((c, c, grid[:, :4], 4, 0, 1, 1), (c, c[:, :8], grid, 4, 0, 1, 1), (c, c, grid, 4, 0, 0, 0), (c, c, grid, 3, 0, 1, 1)):
        with pytest.raises(bbme.BbmeError) as e:
            bbme.compensate_cells_bgr(*args)
        assert e.value.status == _capi.ERR_INVALID


# ---- integer against quarter-pel colour prediction ---------------------------------------------------------------------------
def _psnr(st):
    return 10.0 * math.log10(255.0 ** 2 * 3 * st[2] / st[0])


# (search, block, integer (sse, sad, pixels, skipped), quarter-pel the same): what bbme_compensate_bgr_host gave on this pair when
# the rule was written down; the rule is exact, so these are expected to the last digit
VENUS = [([16] * 3, [8] * 3, (8401477, 843613, 159600, 0), (6801060, 434836, 159600, 0)),
         ([30] * 2, [16] * 2, (10339578, 909940, 159600, 0), (8168346, 478640, 159600, 0))]


@pytest.fixture(scope="module")
def venus_pair_bgr(bbme, venus_flo):
    """tests/test_subpel_compensation_cpu.py's venus_pair with one independent texture per channel: channel c is
    warp_pair_from_flow of the ground truth with seed 4711 + c."""
    gt = bbme.Flow().ReadFlowFile(venus_flo)
    pairs = [bbme.warp_pair_from_flow(gt, seed=4711 + c) for c in range(3)]
    return (gt.shape[1], gt.shape[0], np.ascontiguousarray(np.stack([p[0] for p in pairs], -1)),
            np.ascontiguousarray(np.stack([p[1] for p in pairs], -1)))


@pytest.mark.parametrize("search,block,exp_int,exp_q4", VENUS)
def test_quality_on_the_venus_pair(bbme, oracle, venus_pair_bgr, capsys, search, block, exp_int, exp_q4):
    """The colour prediction of frame 1 along the oracle's integer field of the LUMA planes (unit 1) and along the same field
    refined on the luma planes (bbme_subpel_host; unit 4), statistics over the whole frame."""
    w, h, c1, c2 = venus_pair_bgr
    omf = oracle.OracleMF(np_bgr_to_gray(c1), np_bgr_to_gray(c2), search, block)
    field = omf.calc_motion_block_matching()
    p1, p2 = omf.image(0, 1).copy(), omf.image(0, 2).copy()
    px, py = omf.padding_x, omf.padding_y
    omf.close()
    cells = np.ascontiguousarray(field[::2, ::2]).astype(np.int16)
    q4, _ = bbme.subpel_cells(p1, p2, cells)
    out_int, st_int = bbme.compensate_cells_bgr(c1, c2, cells, 1, 0, px, py)
    out_q4, st_q4 = bbme.compensate_cells_bgr(c1, c2, q4, 4, 0, px, py)
    st_int, st_q4 = stats_of(st_int), stats_of(st_q4)
    for out, st, grid, unit in ((out_int, st_int, cells, 1), (out_q4, st_q4, q4, 4)):
        exp_out, exp_st = np_compensate_bgr(c1, c2, grid, unit, 0, px, py)
        assert np.array_equal(out, exp_out) and st == exp_st
    with capsys.disabled():
        print("\ncolour compensation, Venus pair %dx%d, search %s block %s:\n"
              "  integer cells      sse %d sad %d pixels %d skipped %d -> %.2f dB\n"
              "  quarter-pel cells  sse %d sad %d pixels %d skipped %d -> %.2f dB (sse x %.3f)"
              % ((w, h, search, block) + st_int + (_psnr(st_int),) + st_q4 + (_psnr(st_q4), st_q4[0] / st_int[0])))
    assert st_q4[0] < st_int[0]
    assert st_int == exp_int and st_q4 == exp_q4
