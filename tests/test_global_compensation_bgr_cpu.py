"""The BGR global compensation rule of include/bbme.h on the CPU: bbme_global_compensate_bgr_host against a numpy restatement
written here -- the grey rule's restatement on each channel of the zero-padded view, cropped --, the rule's four properties and
its refusals.  No GPU.  Everything is bit for bit; no tolerance appears."""
import ctypes as C

import numpy as np
import pytest

from test_bgr_cpu import SHAPES
from test_global_motion_cpu import STAT_KEYS, np_global_compensate

NEW_SYMBOLS = ["bbme_global_compensate_bgr_host", "bbme_cells_global_compensate_bgr_device", "bbme_global_compensate_bgr_device",
               "bbme_get_global_compensated_bgr_host", "bbme_global_compensation_error_bgr"]

GEOMETRIES = [(w, h, px, py) for (w, h, _, _), (_, _, px, py) in SHAPES.items()]      # pads (1,1), (1,0), (2,2), (0,0)
PITCH_EXTRA = (0, 1, 5)
FILLS = (0, 3, 255)


# ---- the numpy restatement --------------------------------------------------------------------------------------------------
def np_global_compensate_bgr(c1, c2, model, unit=1, fill=0, pad_x=0, pad_y=0, window=None):
    """The rule in its own words: the grey rule on every channel of the zero-padded view, the unpadded crop of it; statistics
    over the window moved into the padded view, sse and sad added over the channels."""
    c2 = np.asarray(c2, np.uint8)
    h, w = c2.shape[:2]
    win = (0, 0, w, h) if window is None else window
    pwin = (win[0] + pad_x, win[1] + pad_y, win[2], win[3])
    out = np.empty((h, w, 3), np.uint8)
    stats = None
    for c in range(3):
        p2 = np.pad(c2[:, :, c], ((pad_y, pad_y), (pad_x, pad_x)))
        p1 = None if c1 is None else np.pad(np.asarray(c1, np.uint8)[:, :, c], ((pad_y, pad_y), (pad_x, pad_x)))
        o, st = np_global_compensate(p1, p2, model, unit, fill, pwin)
        out[:, :, c] = o[pad_y:pad_y + h, pad_x:pad_x + w]
        if st is not None:
            stats = st if stats is None else (stats[0] + st[0], stats[1] + st[1], stats[2], stats[3])
            assert stats[2:] == st[2:]                                    # pixels and skipped do not depend on the channel
    return out, stats


def source_classes(w, h, px, py, model, unit):
    """Per output pixel: 0 every tap of non-zero weight inside the frame, 1 all of them in the padding (the sample is 0), 2 some
    inside and some in the padding (straddling the frame's edge), 3 not compensated (fill); and the side its source leans to."""
    m = [int(v) for v in model]
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    X, Y = 2 * x + 1 - w, 2 * y + 1 - h
    mul = 4 // unit
    qx = ((m[0] + m[1] * X + m[2] * Y) * mul + 32768) >> 16
    qy = ((m[3] + m[4] * X + m[5] * Y) * mul + 32768) >> 16
    sx, sy = x + (qx >> 2), y + (qy >> 2)
    x1, y1 = ((qx & 3) != 0).astype(np.int64), ((qy & 3) != 0).astype(np.int64)
    ok = (sx >= -px) & (sx + 1 + x1 <= w + px) & (sy >= -py) & (sy + 1 + y1 <= h + py)
    inside = lambda v, n: (v >= 0) & (v < n)                              # noqa: E731
    t = [inside(sx + dx * x1, w) & inside(sy + dy * y1, h) for dx in (0, 1) for dy in (0, 1)]
    every, some = t[0] & t[1] & t[2] & t[3], t[0] | t[1] | t[2] | t[3]
    cls = np.where(~ok, 3, np.where(every, 0, np.where(some, 2, 1)))
    side = {"left": sx < 0, "right": sx + x1 >= w, "top": sy < 0, "bottom": sy + y1 >= h}
    return cls, side


# ---- the cases (the GPU tests use the same) ------------------------------------------------------------------------------------
EDGE_MODEL = ((20000, 2621, -700, -9000, 700, 2621), 1)                   # zoom 8 % and a rotation about the centre, unit 1: at the
                                                                          # frame's edges the sources lie 4 to 6 pixels further out


def models_for(w, h):
    """(model, unit) pairs: identity, whole-pixel translations in the four directions (small, and far enough to read the padding
    and to leave the plane), the 16 quarter-pel fraction pairs, unit 1 offsets that round to each quarter (from below, from above
    and the tie), the edge-straddling affine model in both units, and the int32 extremes."""
    out = [((0, 0, 0, 0, 0, 0), 1), ((0, 0, 0, 0, 0, 0), 4)]
    for tx, ty in ((3, 0), (-3, 0), (0, 2), (0, -2), (w - 1, 0), (-(w - 1), 0), (0, h), (0, -(h + 1)), (-1, 1)):
        for unit in (1, 4):
            out.append(((tx * unit << 16, 0, 0, ty * unit << 16, 0, 0), unit))
    for fx in range(4):
        for fy in range(4):
            out.append((((4 * 1 + fx) << 16, 0, 0, (4 * -2 + fy) << 16, 0, 0), 4))
    for k in range(4):
        for eps in (-3000, 3000, 8192):                                   # q = k, k and k + 1
            out.append(((16384 * k + eps, 0, 0, -(16384 * k + eps), 0, 0), 1))
    out.append(EDGE_MODEL)
    out.append((tuple(4 * v for v in EDGE_MODEL[0]), 4))
    out.append(((-30000, -1900, 500, 40001, -500, -2100), 1))             # shrinking: every source inside, every fraction pair
    out += [((2 ** 31 - 1, 0, 0, 0, 0, 0), 1), ((0, 0, 0, -2 ** 31, 0, 0), 4),
            ((2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1, -2 ** 31), 1),
            ((-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1), 4)]
    return out


def frame_windows(w, h):
    return [None, (1, 1, w - 3, h - 2), (3, 0, 2, h), (w - 1, h - 1, 1, 1), (0, 0, w, h), (0, h - 1, w, 1)]


def pitched(rng, h, w, pitch):
    """A random (h, w, 3) colour frame in a buffer of exactly pitch (h - 1) + 3 w bytes, the gaps random too."""
    buf = rng.integers(0, 256, size=pitch * (h - 1) + 3 * w, dtype=np.uint8)
    return np.lib.stride_tricks.as_strided(buf, (h, w, 3), (pitch, 3, 1))


def host_rule(c1, c2, w, h, px, py, model, unit, fill, window, want_out=True, want_stats=True, out_pitch=None):
    """bbme_global_compensate_bgr_host itself (not the package's wrapper) -> (rc, out or None, stats tuple or None)."""
    from blockbasedmotionestimation_amd import _capi
    out_pitch = 3 * w if out_pitch is None else out_pitch
    out = np.full((h, out_pitch), 0xA5, np.uint8) if want_out else None
    st = (C.c_ulonglong * 4)(*[0xDEAD] * 4) if want_stats else None
    m = np.asarray(model, np.int32)
    win = None if window is None else (C.c_int * 4)(*window)
    rc = _capi.lib().bbme_global_compensate_bgr_host(None if c1 is None else c1.ctypes.data, c2.ctypes.data, w, h, c2.strides[0], px, py,
                                                     m.ctypes.data, unit, fill, win, None if out is None else out.ctypes.data, out_pitch,
                                                     st)
    return rc, out, (tuple(st) if st is not None else None)


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    for name in NEW_SYMBOLS:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    for name in ("draw_MVimage_global_bgr", "compensation_error_global_bgr", "cells_global_compensate_bgr_device"):
        assert hasattr(bbme.MF, name), name
    assert hasattr(bbme.MFBatch, "compensation_errors_global_bgr") and hasattr(bbme.MFChain, "compensation_errors_global_bgr")
    assert hasattr(bbme, "global_compensate_bgr")


@pytest.mark.parametrize("extra", PITCH_EXTRA)
@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_host_rule_equals_numpy(bbme, w, h, px, py, extra):
    rng = np.random.default_rng(1000 * w + 10 * px + extra)
    pitch = 3 * w + extra
    c1, c2 = pitched(rng, h, w, pitch), pitched(rng, h, w, pitch)
    windows = frame_windows(w, h)
    all_skipped = 0
    for n, (model, unit) in enumerate(models_for(w, h)):
        fill, window = FILLS[n % 3], windows[n % len(windows)]
        exp_out, exp_st = np_global_compensate_bgr(c1, c2, model, unit, fill, px, py, window)
        rc, out, st = host_rule(c1, c2, w, h, px, py, model, unit, fill, window, out_pitch=3 * w + (n % 3))
        assert rc == 0
        assert np.array_equal(out[:, :3 * w].reshape(h, w, 3), exp_out), (model, unit, fill)
        assert np.all(out[:, 3 * w:] == 0xA5)                             # nothing written between the rows
        assert st == exp_st, (model, unit, window)
        all_skipped += exp_st[2] == 0
        # out only and statistics only, and the package's wrapper
        rc, out1, none = host_rule(None, c2, w, h, px, py, model, unit, fill, None, want_stats=False)
        assert rc == 0 and none is None and np.array_equal(out1.reshape(h, w, 3), exp_out)
        rc, none, st1 = host_rule(c1, c2, w, h, px, py, model, unit, 255 - fill, window, want_out=False)
        assert rc == 0 and none is None and st1 == exp_st                 # independent of fill
        wout, wst = bbme.global_compensate_bgr(c1, c2, model, unit, fill, px, py, window)
        assert np.array_equal(wout, exp_out) and tuple(wst[k] for k in STAT_KEYS) == exp_st
        if exp_st[2]:
            assert wst["mse"] == exp_st[0] / (3 * exp_st[2])
    assert all_skipped >= 4                                               # the int32 extremes skip everything, without overflow


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_edge_model_meets_padding_edge_and_outside_on_every_side(w, h, px, py):
    """What the edge-straddling model is for: on each side that has padding, sources in the padding (zero), straddling the frame's
    edge and outside the padded plane (fill); on a side without padding the first two cannot exist."""
    for model, unit in (EDGE_MODEL, (tuple(4 * v for v in EDGE_MODEL[0]), 4)):
        cls, side = source_classes(w, h, px, py, model, unit)
        assert (cls == 0).sum() > w * h // 2
        for name, pad in (("left", px), ("right", px), ("top", py), ("bottom", py)):
            assert ((cls == 3) & side[name]).any(), (name, "fill")
            assert ((cls == 2) & side[name]).any() == (pad > 0), (name, "straddle")
            if pad > 1:
                assert ((cls == 1) & side[name]).any(), (name, "padding")
    if px and py:
        cls, _ = source_classes(w, h, px, py, *EDGE_MODEL)
        assert (cls == 1).any()


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_grey_frames_give_the_grey_rule_on_the_padded_plane(bbme, w, h, px, py):
    rng = np.random.default_rng(7 * w + px)
    g1, g2 = rng.integers(0, 256, size=(2, h, w)).astype(np.uint8)
    c1, c2 = np.repeat(g1[:, :, None], 3, 2), np.repeat(g2[:, :, None], 3, 2)
    p1, p2 = bbme.pad_zero(g1, px, py), bbme.pad_zero(g2, px, py)
    for (model, unit), window in zip(models_for(w, h)[::3] + [EDGE_MODEL], frame_windows(w, h) * 8):
        out, st = bbme.global_compensate_bgr(c1, c2, model, unit, 3, px, py, window)
        pwin = None if window is None else (window[0] + px, window[1] + py, window[2], window[3])
        if window is None:
            pwin = (px, py, w, h)
        gout, gst = bbme.global_compensate(p1, p2, model, unit, 3, pwin)
        for c in range(3):
            assert np.array_equal(out[:, :, c], gout[py:py + h, px:px + w]), (model, unit, c)
        assert st["sse"] == 3 * gst["sse"] and st["sad"] == 3 * gst["sad"]
        assert st["pixels"] == gst["pixels"] and st["skipped"] == gst["skipped"]


def test_without_padding_each_channel_is_the_grey_rule(bbme):
    rng = np.random.default_rng(11)
    h, w = 50, 70
    c1, c2 = rng.integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    for model, unit in models_for(w, h)[::2]:
        out, st = bbme.global_compensate_bgr(c1, c2, model, unit, 9)
        sse = sad = 0
        for c in range(3):
            gout, gst = bbme.global_compensate(np.ascontiguousarray(c1[:, :, c]), np.ascontiguousarray(c2[:, :, c]), model, unit, 9)
            assert np.array_equal(out[:, :, c], gout), (model, unit, c)
            sse, sad = sse + gst["sse"], sad + gst["sad"]
            assert (st["pixels"], st["skipped"]) == (gst["pixels"], gst["skipped"])
        assert (st["sse"], st["sad"]) == (sse, sad)


@pytest.mark.parametrize("w,h,px,py", GEOMETRIES)
def test_whole_pixel_translation_and_identity(bbme, w, h, px, py):
    rng = np.random.default_rng(w + h)
    c2 = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    view = np.pad(c2, ((py, py), (px, px), (0, 0)))                       # the padded view
    for unit in (1, 4):
        for tx, ty in ((0, 0), (3, -2), (-7, 5), (w, 0), (-1, h - 1), (w + px - 1, 0), (0, -(h + py)), (-(px + 1), py)):
            out, st = bbme.global_compensate_bgr(c2, c2, (tx * unit << 16, 0, 0, ty * unit << 16, 0, 0), unit, 77, px, py)
            ys, xs = np.mgrid[0:h, 0:w]
            sy, sx = ys + py + ty, xs + px + tx
            ok = (sy >= 0) & (sy < h + 2 * py) & (sx >= 0) & (sx < w + 2 * px)
            exp = np.full((h, w, 3), 77, np.uint8)
            exp[ok] = view[sy[ok], sx[ok]]
            assert np.array_equal(out, exp), (unit, tx, ty)
            assert st["pixels"] == int(ok.sum()) and st["skipped"] == h * w - int(ok.sum())
            if (tx, ty) == (0, 0):
                assert np.array_equal(out, c2) and st["sse"] == 0 and st["skipped"] == 0


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    f = _capi.lib().bbme_global_compensate_bgr_host
    w, h = 20, 16
    c = np.zeros((h, w, 3), np.uint8)
    out = np.zeros((h, w, 3), np.uint8)
    big = np.zeros((2, 3 * 8190), np.uint8)
    model = np.zeros(6, np.int32)
    st = (C.c_ulonglong * 4)()
    win = lambda *v: (C.c_int * 4)(*v)                                    # noqa: E731
    p, o, m = c.ctypes.data, out.ctypes.data, model.ctypes.data
    bad = [
        f(p, None, w, h, 3 * w, 1, 1, m, 1, 0, None, o, 3 * w, st),       # no frame 2
        f(p, p, w, h, 3 * w, 1, 1, None, 1, 0, None, o, 3 * w, st),       # no model
        f(p, p, w, h, 3 * w, 1, 1, m, 1, 0, None, None, 3 * w, None),     # neither out nor statistics
        f(None, p, w, h, 3 * w, 1, 1, m, 1, 0, None, None, 3 * w, st),    # statistics without frame 1
        f(p, p, 0, h, 3 * w, 1, 1, m, 1, 0, None, o, 3 * w, st),
        f(p, p, w, h, 3 * w, -1, 1, m, 1, 0, None, o, 3 * w, st),
        f(p, p, w - 1, h, 3 * w, 1, 1, m, 1, 0, None, o, 3 * w, st),      # the padded view is odd
        f(p, p, w, h, 3 * w, 1, 1, m, 2, 0, None, o, 3 * w, st),          # unit
        f(p, p, w, h, 3 * w, 1, 1, m, 1, 256, None, o, 3 * w, st),        # fill
        f(p, p, w, h, 3 * w, 1, 1, m, 1, -1, None, o, 3 * w, st),
        f(p, p, w, h, 3 * w - 1, 1, 1, m, 1, 0, None, o, 3 * w, st),      # colour pitch
        f(p, p, w, h, 3 * w, 1, 1, m, 1, 0, None, o, 3 * w - 1, st),      # output pitch
        f(p, p, w, h, 3 * w, 1, 1, m, 1, 0, win(0, 0, w + 1, 1), o, 3 * w, st),      # the window is in FRAME pixels
        f(p, p, w, h, 3 * w, 1, 1, m, 1, 0, win(-1, 0, 2, 1), o, 3 * w, st),
        f(p, p, w, h, 3 * w, 1, 1, m, 1, 0, win(0, 0, 0, 1), o, 3 * w, st),
    ]
    assert bad == [-1] * len(bad), bad
    assert f(None, big.ctypes.data, 8190, 2, 3 * 8190, 0, 0, m, 1, 0, None, big.ctypes.data, 3 * 8190, None) == _capi.ERR_UNSUPPORTED
    assert f(None, big.ctypes.data, 8188, 2, 3 * 8190, 1, 0, m, 1, 0, None, big.ctypes.data, 3 * 8190, None) == _capi.ERR_UNSUPPORTED
    assert f(None, p, w, h, 3 * w, 1, 1, m, 1, 0, None, o, 3 * w, None) == 0          # frame 1 may be null without statistics
    assert f(p, p, w, h, 3 * w, 1, 1, m, 1, 0, None, None, 0, st) == 0                # out may be null with statistics
