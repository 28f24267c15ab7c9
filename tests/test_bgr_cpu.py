"""CPU tests of colour video (include/bbme.h, "LUMA RULE" and "BGR INTERPOLATION RULE"): the C-ABI exports the colour calls;
bbme_bgr_to_gray_host and bbme_interpolate_bgr_host follow the two rules, which are restated here in numpy from the header's text
and imported by the GPU tests; on frames with B = G = R every channel is the grey rule's frame; on a colour video of constant
motion the interpolated middle frame beats the average of its neighbours in every channel."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_bidirectional import _oracle_fields
from test_interpolation_cpu import _box5, np_interpolate, psnr, random_grids

NEW_SYMBOLS = ["bbme_bgr_to_gray_host", "bbme_set_frames_host_bgr", "bbme_set_frames_host_bgr_async", "bbme_set_frames_device_bgr",
               "bbme_set_chain_frames_host_bgr", "bbme_set_chain_frames_host_bgr_async", "bbme_set_chain_frames_device_bgr",
               "bbme_bgr_frames_device_pair", "bbme_cells_interpolate_bgr_device", "bbme_interpolate_bgr_device",
               "bbme_get_interpolated_bgr_host", "bbme_interpolate_bgr_host"]

# (width, height, search, block): (padded width, padded height, pad_x, pad_y) by bbme_plan_padding's arithmetic.  Both paddings
# odd and a last run of 2 cells (CW = 66); an odd pad_x alone; even paddings and whole runs; no padding and CW = 66.
SHAPES = {
    (130, 98, (12,), (4,)): (132, 100, 1, 1),
    (130, 100, (12,), (4,)): (132, 100, 1, 0),
    (124, 100, (12,), (8,)): (128, 104, 2, 2),
    (132, 100, (12,), (2,)): (132, 100, 0, 0),
}
PHASES = [(1, 2), (1, 3), (3, 4), (255, 256)]


def np_bgr_to_gray(frame):
    """The luma rule: Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 of a (..., 3) B,G,R array."""
    f = np.asarray(frame).astype(np.int64)
    return ((1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + 8192) >> 14).astype(np.uint8)


def np_pad_zero(img, pad_x, pad_y):
    return np.pad(img, ((pad_y, pad_y), (pad_x, pad_x)))


def np_interpolate_bgr(I1, I2, C1, C2, F, B, num, den, pad_x, pad_y):
    """The BGR interpolation rule: the selection is the interpolation rule's on the padded luma planes I1, I2 (np_interpolate's
    map; v = F, -B or 0 of the cell accordingly); output pixel (x, y) of the W x H frame has the padded position (X, Y) =
    (x + pad_x, y + pad_y), its cell is (X >> 1, Y >> 1) with origin o, s = floor((num v + den // 2) / den), p1 = o - s,
    q1 = p1 + (X & 1, Y & 1) - (pad_x, pad_y), q2 = q1 + v, a pixel outside the frame reads 0, and per channel
    out = ((den - num) C1[q1] + num C2[q2] + den // 2) // den."""
    _, sel, _ = np_interpolate(I1, I2, F, B, num, den)
    H, W = C1.shape[:2]
    assert I1.shape == (H + 2 * pad_y, W + 2 * pad_x)
    v = np.where(sel[..., None] == 0, np.asarray(F).astype(np.int64), 0)
    if B is not None:
        v = np.where(sel[..., None] == 1, -np.asarray(B).astype(np.int64), v)
    y, x = np.mgrid[0:H, 0:W]
    X, Y = x + pad_x, y + pad_y
    cx, cy = X >> 1, Y >> 1
    vx, vy = v[cy, cx, 0], v[cy, cx, 1]
    q1x = 2 * cx - (num * vx + den // 2) // den + (X & 1) - pad_x           # numpy's // floors
    q1y = 2 * cy - (num * vy + den // 2) // den + (Y & 1) - pad_y
    q2x, q2y = q1x + vx, q1y + vy

    def texel(img, qx, qy):
        inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        return np.where(inside[..., None], np.asarray(img).astype(np.int64)[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)], 0)

    return (((den - num) * texel(C1, q1x, q1y) + num * texel(C2, q2x, q2y) + den // 2) // den).astype(np.uint8)


def colour_pair(w, h, seed):
    """Two random colour frames with a patch of one flat colour in both (there every hypothesis costs the same: ties)."""
    rng = np.random.default_rng(seed)
    c1 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    c2 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for c in (c1, c2):
        c[h // 4:h // 2, w // 3:2 * w // 3] = (40, 170, 90)
    return c1, c2


def luma_planes(c1, c2, pad_x, pad_y):
    return np_pad_zero(np_bgr_to_gray(c1), pad_x, pad_y), np_pad_zero(np_bgr_to_gray(c2), pad_x, pad_y)


def constant_motion_bgr_video(w, h, seed, mm, tiles):
    """Three colour frames: three band-limited textures of different seeds, one per channel, whose tiles x tiles tiles all move by
    the same constant vector per frame (components in -mm // 2 .. mm // 2), frames 1 and 2 with +-2 noise: frame 1 is the true
    middle of frames 0 and 2 (tests/test_interpolation_cpu.py's constant_motion_video, in colour)."""
    m = 2 * mm
    mv = np.random.default_rng(seed + 1).integers(-mm // 2, mm // 2 + 1, size=(tiles, tiles, 2))
    ty = np.minimum(np.arange(h) * tiles // h, tiles - 1)
    tx = np.minimum(np.arange(w) * tiles // w, tiles - 1)
    mo = mv[ty[:, None], tx[None, :]]
    ys, xs = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed + 2)
    frames = [np.empty((h, w, 3), np.uint8) for _ in range(3)]
    for ch in range(3):
        base = np.random.default_rng(seed + 100 * (ch + 1)).integers(0, 256, size=(h + 2 * m, w + 2 * m)).astype(np.float64)
        for _ in range(3):
            base = _box5(base)
        base -= base.min()
        base *= 255 / base.max()
        base = np.rint(base).astype(np.uint8)
        for k in (0, 1, 2):
            f = base[ys - k * mo[..., 1] + m, xs - k * mo[..., 0] + m].astype(np.int16)
            if k > 0:
                f = f + noise.integers(-2, 3, size=f.shape)
            frames[k][..., ch] = np.clip(f, 0, 255)
    return frames


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
        assert "int %s(" % name in header, name
    assert "LUMA RULE" in header and "BGR INTERPOLATION RULE" in header
    for name in ("bgr_to_gray", "interpolate_cells_bgr"):
        assert callable(getattr(bbme, name)) and name in bbme.__all__
    for name in ("interpolate_bgr", "interpolate_run_bgr", "cells_interpolate_bgr_device"):
        assert callable(getattr(bbme.MF, name))
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    table = (C.c_void_p * 1)(buf.ctypes.data)
    d = buf.ctypes.data
    inv = _capi.ERR_INVALID
    # a null context is refused before anything touches a device
    assert L.bbme_set_frames_host_bgr(None, 0, d, d, 12) == inv
    assert L.bbme_set_frames_host_bgr_async(None, 0, d, d, 12) == inv
    assert L.bbme_set_frames_device_bgr(None, 0, d, d, 12) == inv
    assert L.bbme_set_chain_frames_host_bgr(None, 0, 1, table, 12) == inv
    assert L.bbme_set_chain_frames_host_bgr_async(None, 0, 1, table, 12) == inv
    assert L.bbme_set_chain_frames_device_bgr(None, 0, 1, table, 12) == inv
    assert L.bbme_bgr_frames_device_pair(None, 0, C.byref(C.c_void_p()), C.byref(C.c_void_p())) == inv
    assert L.bbme_cells_interpolate_bgr_device(None, 0, d, d, d, d, 12, 1, 1, 2, d, 12, 0, None) == inv
    assert L.bbme_interpolate_bgr_device(None, 0, 1, 1, 2, d, 12, 0, None) == inv
    assert L.bbme_get_interpolated_bgr_host(None, 0, 1, 2, d) == inv


def test_the_issue_shapes_pad_as_stated(bbme):
    for (w, h, search, block), exp in SHAPES.items():
        assert bbme.plan_padding(w, h, list(search), list(block)) == exp


def test_bgr_to_gray_follows_the_luma_rule(bbme):
    from blockbasedmotionestimation_amd import _capi
    rng = np.random.default_rng(31)
    wide = rng.integers(0, 256, (37, 53 + 5, 3), dtype=np.uint8)
    frame = wide[:, :53]                                    # rows 3 * 58 bytes apart: a pitch above 3 W, read in place
    assert frame.strides[0] > 3 * 53
    assert np.array_equal(bbme.bgr_to_gray(frame), np_bgr_to_gray(frame))
    # a pitch of 3 W + 1 through the C-ABI
    w, h = 21, 9
    raw = rng.integers(0, 256, h * (3 * w + 1), dtype=np.uint8)
    rows = np.stack([raw[y * (3 * w + 1):y * (3 * w + 1) + 3 * w].reshape(w, 3) for y in range(h)])
    out = np.empty((h, w), np.uint8)
    assert _capi.lib().bbme_bgr_to_gray_host(raw.ctypes.data, w, h, 3 * w + 1, out.ctypes.data) == 0
    assert np.array_equal(out, np_bgr_to_gray(rows))
    # every grey level is kept exactly
    g = np.arange(256, dtype=np.uint8)
    grey = np.repeat(g[None, :, None], 3, axis=2)
    assert np.array_equal(bbme.bgr_to_gray(grey)[0], g)
    # the eight corner colours, written out: B, G, R weights 1868, 9617, 4899 of 16384, rounded
    corners = np.array([[(b, gg, r) for b in (0, 255) for gg in (0, 255) for r in (0, 255)]], np.uint8)
    exp = [0, 76, 150, 226, 29, 105, 179, 255]
    assert bbme.bgr_to_gray(corners)[0].tolist() == exp == np_bgr_to_gray(corners)[0].tolist()
    src = raw.ctypes.data
    for bad in ((None, 4, 4, 12), (src, 0, 4, 12), (src, 4, 0, 12), (src, 4, 4, 11)):
        assert _capi.lib().bbme_bgr_to_gray_host(*bad, out.ctypes.data) == _capi.ERR_INVALID, bad
    assert _capi.lib().bbme_bgr_to_gray_host(src, 4, 4, 12, None) == _capi.ERR_INVALID


@pytest.mark.parametrize("shape", list(SHAPES))
def test_interpolate_bgr_host_equals_numpy(bbme, shape):
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    c1, c2 = colour_pair(w, h, 7 * w + h)
    I1, I2 = luma_planes(c1, c2, px, py)
    assert np.array_equal(I1, bbme.pad_zero(bbme.bgr_to_gray(c1), px, py))
    rng = np.random.default_rng(w + h)
    f, b = random_grids(H0 // 2, W0 // 2, rng)
    ties = 0
    for num, den in PHASES:
        for bwd in (b, None):
            exp = np_interpolate_bgr(I1, I2, c1, c2, f, bwd, num, den, px, py)
            got = bbme.interpolate_cells_bgr(I1, I2, c1, c2, f, bwd, num, den, px, py)
            assert got.shape == (h, w, 3) and np.array_equal(got, exp), (num, den, bwd is not None)
        _, sel, _ = np_interpolate(I1, I2, f, b, num, den)
        ties += int((sel[H0 // 8 + 2:H0 // 4 - 2, W0 // 6 + 2:W0 // 3 - 2] == 0).sum())
    assert ties > 0                                          # inside the flat patch the first hypothesis won ties


def test_interpolate_bgr_host_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    lum = np.zeros((12, 16), np.uint8)
    col = np.zeros((10, 14, 3), np.uint8)
    g = np.zeros((6, 8, 2), np.int16)
    out = np.zeros((10, 14, 3), np.uint8)

    def call(l1=lum, c1=col, pw=16, ph=12, w=14, h=10, px=1, py=1, fwd=g, num=1, den=2, o=out):
        p = lambda a: None if a is None else a.ctypes.data
        return L.bbme_interpolate_bgr_host(p(l1), p(lum), pw, ph, p(c1), p(col), w, h, px, py, p(fwd), None, num, den, p(o))

    assert call() == 0
    for kw in (dict(l1=None), dict(c1=None), dict(fwd=None), dict(o=None), dict(px=0), dict(py=2), dict(w=15), dict(px=-1, w=18),
               dict(num=0), dict(num=2), dict(den=257, num=1), dict(den=1)):
        assert call(**kw) == _capi.ERR_INVALID, kw


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gray_frames_give_the_grey_result_in_every_channel(bbme, shape):
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    rng = np.random.default_rng(3 * w + h)
    g1, g2 = (rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2))
    g1[h // 4:h // 2, w // 3:2 * w // 3] = g2[h // 4:h // 2, w // 3:2 * w // 3] = 99
    c1, c2 = (np.repeat(g[..., None], 3, axis=2) for g in (g1, g2))
    assert np.array_equal(bbme.bgr_to_gray(c1), g1)
    I1, I2 = bbme.pad_zero(g1, px, py), bbme.pad_zero(g2, px, py)
    f, b = random_grids(H0 // 2, W0 // 2, rng)
    for num, den in PHASES:
        for bwd in (b, None):
            grey = bbme.interpolate_cells(I1, I2, f, bwd, num, den)[0][py:py + h, px:px + w]
            got = bbme.interpolate_cells_bgr(I1, I2, c1, c2, f, bwd, num, den, px, py)
            for ch in range(3):
                assert np.array_equal(got[..., ch], grey), (num, den, bwd is not None, ch)


@pytest.mark.parametrize("case", [(128, 96, (48, 48), (16, 16), 11, 12, 1), (192, 128, (40, 40), (8, 8), 13, 8, 3)])
def test_interpolated_colour_middle_frame_beats_the_average(bbme, oracle, case):
    """Estimate the lumas of (f0, f2) both ways with the oracle and interpolate the colour frames at 1 / 2: over the interior the
    PSNR against the true middle frame f1 is higher than the rounded average's in EVERY channel -- a condition, no fitted number.
    Gains this test prints: one tile B +17.3, G +18.9, R +19.6 dB; 3 x 3 tiles B +9.7, G +10.5, R +9.9 dB."""
    w, h, search, block, seed, mm, tiles = case
    search, block = list(search), list(block)
    f0, f1, f2 = constant_motion_bgr_video(w, h, seed, mm, tiles)
    y0, y2 = bbme.bgr_to_gray(f0), bbme.bgr_to_gray(f2)
    _, fwd = _oracle_fields(bbme, oracle, y0, y2, search, block)
    _, bwd = _oracle_fields(bbme, oracle, y2, y0, search, block)
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    I1, I2 = bbme.pad_zero(y0, px, py), bbme.pad_zero(y2, px, py)
    mid = bbme.interpolate_cells_bgr(I1, I2, f0, f2, fwd, bwd, 1, 2, px, py)
    assert np.array_equal(mid, np_interpolate_bgr(I1, I2, f0, f2, fwd, bwd, 1, 2, px, py))
    avg = ((f0.astype(np.int32) + f2 + 1) // 2).astype(np.uint8)
    inner = (slice(mm, h - mm), slice(mm, w - mm))
    for ch, name in enumerate("BGR"):
        p_rule, p_avg = psnr(mid[inner][..., ch], f1[inner][..., ch]), psnr(avg[inner][..., ch], f1[inner][..., ch])
        print("case %s channel %s: rule %.1f dB, average %.1f dB, gain %+.1f dB" % (case, name, p_rule, p_avg, p_rule - p_avg))
        assert p_rule > p_avg, (name, p_rule, p_avg)
