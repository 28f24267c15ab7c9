"""CPU tests of the subpel compensation rule (include/bbme.h, "SUBPEL COMPENSATION RULE"): the C-ABI exports the new calls;
bbme_subpel_compensate_host follows the rule, which is restated here in vectorised numpy from the header's text (the four-term
sample, taps of weight 0 not read) and imported by the GPU tests; with Q = 4 G it is the integer compensation rule bit for bit;
on the Venus pair the prediction along the refined field of the oracle's estimate gains about 2 dB over the integer one."""
import ctypes as C
import math
import os

import numpy as np
import pytest

NEW_SYMBOLS = ["bbme_subpel_compensate_host", "bbme_cells_subpel_compensate_device", "bbme_subpel_compensate_device",
               "bbme_get_subpel_compensated_host", "bbme_subpel_compensation_error"]

STAT_KEYS = ("sse", "sad", "pixels", "skipped")
SIZES = ((24, 16), (38, 26), (200, 136))
FILLS = (0, 7, 255)


def np_subpel_compensate(I1, I2, Q, fill=0, window=None):
    """The rule of include/bbme.h -> (frame uint8 (H0, W0), (sse, sad, pixels, skipped) over window (x0, y0, w, h) in pixels,
    None = the whole plane).  I1 may be None: the statistics are then None."""
    I2 = np.asarray(I2).astype(np.int64)
    Q = np.asarray(Q).astype(np.int64)
    H0, W0 = I2.shape
    CH, CW = H0 // 2, W0 // 2
    assert Q.shape == (CH, CW, 2)
    cy, cx = np.mgrid[0:CH, 0:CW]
    qx, qy = Q[..., 0], Q[..., 1]
    ix, iy, fx, fy = qx >> 2, qy >> 2, qx & 3, qy & 3
    sx, sy = 2 * cx + ix, 2 * cy + iy
    ok = (0 <= sx) & (sx + 2 + (fx != 0) <= W0) & (0 <= sy) & (sy + 2 + (fy != 0) <= H0)
    mc = np.full((H0, W0), fill, np.int64)
    for k in range(2):
        for j in range(2):
            acc = np.full((CH, CW), 8, np.int64)
            for dx, dy, wgt in ((0, 0, (4 - fx) * (4 - fy)), (1, 0, fx * (4 - fy)), (0, 1, (4 - fx) * fy), (1, 1, fx * fy)):
                use = ok & (wgt != 0)                          # a tap of weight 0 is not part of the sample
                y, x = np.where(use, sy + k + dy, 0), np.where(use, sx + j + dx, 0)
                assert ((0 <= y) & (y < H0) & (0 <= x) & (x < W0)).all()
                acc += np.where(use, wgt * I2[y, x], 0)
            mc[2 * cy + k, 2 * cx + j] = np.where(ok, acc >> 4, fill)
    assert mc.min() >= 0 and mc.max() <= 255
    if I1 is None:
        return mc.astype(np.uint8), None
    x0, y0, w, h = window if window is not None else (0, 0, W0, H0)
    inside = np.zeros((H0, W0), bool)
    inside[y0:y0 + h, x0:x0 + w] = True
    okp = ok.repeat(2, 0).repeat(2, 1)
    d = (mc - np.asarray(I1).astype(np.int64))[inside & okp]
    stats = (int((d * d).sum()), int(np.abs(d).sum()), int(d.size), int((inside & ~okp).sum()))
    return mc.astype(np.uint8), stats


def host(bbme, I1, I2, Q, fill=0, window=None):
    mc, st = bbme.compensate_cells_subpel(I1, I2, Q, fill, window)
    return mc, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, I1, I2, Q, fill=0, window=None, what=None):
    exp = np_subpel_compensate(I1, I2, Q, fill, window)
    got = host(bbme, I1, I2, Q, fill, window)
    assert np.array_equal(got[0], exp[0]), (what, fill, window, np.argwhere(got[0] != exp[0])[:4])
    assert got[1] == exp[1], (what, fill, window, got[1], exp[1])
    return exp


def planes(w, h, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, size=(2, h, w)).astype(np.uint8)
    return a, b


def fraction_grid(w, h, seed, reach=3):
    """Random vectors of a few pixels whose fractions go through all 16 (fx, fy) along the cells, so some leave the plane at
    its edges"""
    rng = np.random.default_rng(seed)
    CH, CW = h // 2, w // 2
    cy, cx = np.mgrid[0:CH, 0:CW]
    k = (cy * CW + cx + seed) % 16
    Q = 4 * rng.integers(-reach, reach + 1, size=(CH, CW, 2)) + np.stack([k & 3, k >> 2], -1)
    assert len({(int(a) & 3, int(b) & 3) for a, b in Q.reshape(-1, 2)}) == 16
    return Q.astype(np.int16)


def edge_grid(w, h, seed):
    """Cells whose s.x takes each of -1, 0, W0 - 3, W0 - 2, W0 - 1 with fx = 0 and with fx != 0, and the same for y; the other
    component and the other cells are random and small -> (grid, [(cx, cy, compensated)])"""
    rng = np.random.default_rng(seed)
    CH, CW = h // 2, w // 2
    Q = (4 * rng.integers(-1, 2, size=(CH, CW, 2)) + rng.integers(0, 4, size=(CH, CW, 2))).astype(np.int64)
    cells = []
    slots = [(cx, cy) for cy in range(1, CH - 1) for cx in range(1, CW - 1)]
    order = rng.permutation(len(slots))
    cases = [(axis, s, f) for axis in (0, 1) for s in ("m1", "0", "n3", "n2", "n1") for f in (0, 1, 2, 3)]
    assert len(slots) >= len(cases)
    for n, (axis, s, f) in enumerate(cases):
        cx, cy = slots[order[n]]
        lim = (w, h)[axis]
        target = {"m1": -1, "0": 0, "n3": lim - 3, "n2": lim - 2, "n1": lim - 1}[s]
        o = 2 * (cx, cy)[axis]
        Q[cy, cx, axis] = 4 * (target - o) + f
        Q[cy, cx, 1 - axis] = 0                                # the other axis stays inside: this one decides
        ok = 0 <= target and target + 2 + (f != 0) <= lim
        cells.append((cx, cy, ok))
    assert np.abs(Q).max() < 32768
    return Q.astype(np.int16), cells


def extreme_grid(w, h, seed):
    rng = np.random.default_rng(seed)
    CH, CW = h // 2, w // 2
    Q = rng.integers(-13, 14, size=(CH, CW, 2)).astype(np.int16)
    ext = np.array([-32768, 32767, -32765, 32764, 0, 3, -1], np.int16)
    pick = rng.random((CH, CW)) < 0.3
    Q[pick] = ext[rng.integers(0, len(ext), size=(int(pick.sum()), 2))]
    Q[0, 0] = (-32768, 32767)
    Q[CH - 1, CW - 1] = (32767, -32768)
    return Q


def odd_windows(w, h):
    return ((1, 1, w - 3, h - 3), (3, 5, 7, 9), (w - 1, h - 1, 1, 1), (5, 3, 1, 1), (0, 1, w, 1), (1, 0, 1, h))


@pytest.mark.parametrize("w,h", SIZES)
def test_host_rule_equals_numpy(bbme, w, h):
    I1, I2 = planes(w, h, w)
    ref = None
    for fill in FILLS:
        for seed in (1, 2):
            Q = fraction_grid(w, h, seed)
            _, st = assert_host_equals_numpy(bbme, I1, I2, Q, fill, None, "fractions")
            assert st[2] > 0 and st[3] > 0 and st[2] + st[3] == w * h
        E = extreme_grid(w, h, 5)
        _, st = assert_host_equals_numpy(bbme, I1, I2, E, fill, None, "int16 extremes")
        assert st[3] >= 8
        Q = fraction_grid(w, h, 3)
        per_fill = [assert_host_equals_numpy(bbme, I1, I2, Q, fill, win, "window")[1] for win in odd_windows(w, h)]
        assert ref is None or per_fill == ref                  # the statistics do not depend on fill
        ref = per_fill
    assert ref[2][2] + ref[2][3] == 1 and ref[3][2] + ref[3][3] == 1         # the windows of one pixel
    # a window that cuts cells counts pixels, not cells; three windows that tile the plane add up
    whole = host(bbme, I1, I2, Q)[1]
    parts = [host(bbme, I1, I2, Q, 0, win)[1] for win in ((0, 0, 5, h), (5, 0, w - 5, 7), (5, 7, w - 5, h - 7))]
    assert tuple(np.sum(parts, 0)) == whole


@pytest.mark.parametrize("w,h", SIZES)
def test_validity_at_every_edge(bbme, w, h):
    I1, I2 = planes(w, h, 7 + w)
    Q, cells = edge_grid(w, h, 11)
    for fill in (7, 255):
        mc, _ = assert_host_equals_numpy(bbme, I1, I2, Q, fill, None, "edges")
        for cx, cy, ok in cells:
            st = host(bbme, I1, I2, Q, fill, (2 * cx, 2 * cy, 2, 2))[1]
            assert (st[2], st[3]) == ((4, 0) if ok else (0, 4)), (cx, cy, ok, Q[cy, cx])
            if not ok:
                assert (mc[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2] == fill).all()
    assert {ok for _, _, ok in cells} == {True, False}


@pytest.mark.parametrize("w,h", SIZES)
def test_integer_vectors_are_the_compensation_rule(bbme, w, h):
    """The anchor: Q = 4 G gives bbme_motion_compensate_host(grid_block 2, block 2), frame and statistics"""
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    I1, I2 = planes(w, h, 3 * w)
    rng = np.random.default_rng(h)
    for reach in (2, 9):
        G = rng.integers(-reach, reach + 1, size=(h // 2, w // 2, 2)).astype(np.int16)
        for fill, win in ((0, None), (7, (1, 3, w - 4, h - 5)), (255, (w - 1, 0, 1, 1))):
            exp = np.empty((h, w), np.uint8)
            s4 = (C.c_ulonglong * 4)()
            cwin = None if win is None else (C.c_int * 4)(*win)
            assert L.bbme_motion_compensate_host(I1.ctypes.data, I2.ctypes.data, w, h, G.ctypes.data, 2, 2, fill, cwin,
                                                 exp.ctypes.data, s4) == 0
            mc, st = host(bbme, I1, I2, (4 * G).astype(np.int16), fill, win)
            assert np.array_equal(mc, exp) and st == tuple(s4), (reach, fill, win)
            if win is None:
                assert st[3] > 0                               # some vectors leave the plane
            assert np_subpel_compensate(I1, I2, 4 * G.astype(np.int64), fill, win)[1] == tuple(s4)


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    H, W = 12, 16
    img = np.zeros((H, W), np.uint8)
    q = np.zeros((H // 2, W // 2, 2), np.int16)
    out = np.zeros((H, W), np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    I, Q = img.ctypes.data, q.ctypes.data

    def call(a=I, b=I, w=W, h=H, q4=Q, fill=0, win=None, o=out.ctypes.data, t=st):
        return L.bbme_subpel_compensate_host(a, b, w, h, q4, fill, win, o, t)

    assert call() == 0
    assert call(b=None) == inv and call(q4=None) == inv
    assert call(o=None, t=None) == inv                                            # nothing asked for
    assert call(a=None) == inv                                                    # statistics without image1
    assert call(a=None, t=None) == 0 and call(o=None) == 0 and call(t=None) == 0
    assert call(w=W - 1) == inv and call(h=H - 1) == inv                          # odd sizes
    assert call(w=0) == inv and call(h=0) == inv
    assert call(fill=-1) == inv and call(fill=256) == inv and call(fill=255) == 0
    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (W - 1, 0, 2, 2), (0, H - 1, 2, 2), (0, 0, W + 1, H)):
        assert call(win=(C.c_int * 4)(*win)) == inv, win
    assert call(win=(C.c_int * 4)(W - 1, H - 1, 1, 1)) == 0
    for args in ((img, img, q[:, :4]), (img, img[:, :8], q)):
        with pytest.raises(bbme.BbmeError) as e:
            bbme.compensate_cells_subpel(*args)
        assert e.value.status == inv


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
        assert "int %s(" % name in header, name
    assert "SUBPEL COMPENSATION RULE" in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_subpel_compensate_device(None, d, d, d, 4, 0, None, d, 8, st, None) == inv
    assert L.bbme_subpel_compensate_device(None, 0, 0, 0, d, 8, None) == inv
    assert L.bbme_get_subpel_compensated_host(None, 0, 0, 0, d) == inv
    assert L.bbme_subpel_compensation_error(None, 0, None, st) == inv
    assert "compensate_cells_subpel" in bbme.__all__ and hasattr(bbme, "compensate_cells_subpel")
    for name in ("draw_MVimage_subpel", "compensation_error_subpel", "cells_compensate_subpel_device"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        for name in ("get_pair_motion_compensated_subpel", "compensation_errors_subpel"):
            assert hasattr(cls, name), name


def _psnr(st):
    return 10.0 * math.log10(255.0 ** 2 * st[2] / st[0])


# (search, block, integer (sse, sad, pixels, skipped), quarter-pel the same): what a numpy restatement of the rule gave on this
# pair when the rule was written down; the rule is exact, so these are expected to the last digit
VENUS = [([16] * 3, [8] * 3, (1709021, 246141, 159600, 0), (1049613, 108945, 159600, 0)),
         ([30] * 2, [16] * 2, (2154733, 263347, 159600, 0), (1428465, 120533, 159600, 0))]


@pytest.fixture(scope="module")
def venus_pair(bbme, venus_flo):
    gt = bbme.Flow().ReadFlowFile(venus_flo)
    return gt.shape[1], gt.shape[0], bbme.warp_pair_from_flow(gt)


@pytest.mark.parametrize("search,block,exp_int,exp_q4", VENUS)
def test_quality_on_the_venus_pair(bbme, oracle, venus_pair, capsys, search, block, exp_int, exp_q4):
    """The pair of tests/test_subpel_cpu.py::test_quality_on_the_venus_pair (420 x 380), built the same way: the prediction of
    frame 1 along the oracle's integer field (bbme_motion_compensate_host, block 2) and along the same field refined
    (bbme_subpel_host), statistics over the unpadded frame."""
    from blockbasedmotionestimation_amd import _capi
    w, h, (f1, f2) = venus_pair
    omf = oracle.OracleMF(f1, f2, search, block)
    field = omf.calc_motion_block_matching()
    p1, p2 = omf.image(0, 1).copy(), omf.image(0, 2).copy()
    px, py = omf.padding_x, omf.padding_y
    omf.close()
    cells = np.ascontiguousarray(field[::2, ::2]).astype(np.int16)
    H0, W0 = p1.shape
    win = (px, py, w, h)
    s4 = (C.c_ulonglong * 4)()
    assert _capi.lib().bbme_motion_compensate_host(p1.ctypes.data, p2.ctypes.data, W0, H0, cells.ctypes.data, 2, 2, 0,
                                                   (C.c_int * 4)(*win), None, s4) == 0
    st_int = tuple(s4)
    q4, _ = bbme.subpel_cells(p1, p2, cells)
    _, st_q4 = assert_host_equals_numpy(bbme, p1, p2, q4, 0, win, "venus")
    assert host(bbme, p1, p2, (4 * cells).astype(np.int16), 0, win)[1] == st_int
    with capsys.disabled():
        print("\nsubpel compensation, Venus pair %dx%d, search %s block %s:\n"
              "  integer cells      sse %d sad %d pixels %d skipped %d -> %.2f dB\n"
              "  quarter-pel cells  sse %d sad %d pixels %d skipped %d -> %.2f dB (sse x %.3f)"
              % ((w, h, search, block) + st_int + (_psnr(st_int),) + st_q4 + (_psnr(st_q4), st_q4[0] / st_int[0])))
    assert st_int[3] == 0 and st_q4[3] == 0
    assert st_q4[0] <= 0.70 * st_int[0]
    assert _psnr(st_q4) - _psnr(st_int) >= 1.5
    assert st_int == exp_int and st_q4 == exp_q4
