"""CPU tests of the forward-backward consistency rule (include/bbme.h, "CONSISTENCY RULE"): the C-ABI exports the direction,
the bidirectional estimate and the consistency calls; bbme_cells_consistency_host follows the rule, which is restated here in
vectorised numpy from the header's text and imported by the GPU tests; hand-made cases carry their answers written out."""
import ctypes as C

import numpy as np
import pytest

from helpers import INT16_SPECIALS

NEW_SYMBOLS = ["bbme_set_direction", "bbme_get_direction", "bbme_estimate_bidirectional", "bbme_backward_cells_device_pair",
               "bbme_get_backward_cells_host_pair", "bbme_cells_consistency_device", "bbme_get_consistency_host",
               "bbme_consistency_stats", "bbme_cells_consistency_host"]

STAT_KEYS = ("consistent", "inconsistent", "outside", "discrepancy")


def np_cells_consistency(a, b, tol, window=None):
    """The rule of include/bbme.h: cell (cx, cy) with (dx, dy) = a[cy, cx] looks at pixel (tx, ty) = (2 cx + dx, 2 cy + dy);
    outside the 2 CW x 2 CH plane: class 2; otherwise (ex, ey) = b[ty >> 1, tx >> 1], d = |dx + ex| + |dy + ey|, class 0 if
    d <= tol else 1.  Returns (mask uint8 (CH, CW), (cells of class 0, 1, 2, sum of d over classes 0 and 1) over window
    (cx0, cy0, cw, ch) in cells, None = all cells)."""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    CH, CW = a.shape[:2]
    cy, cx = np.mgrid[0:CH, 0:CW]
    tx, ty = 2 * cx + a[..., 0], 2 * cy + a[..., 1]
    inside = (tx >= 0) & (ty >= 0) & (tx < 2 * CW) & (ty < 2 * CH)
    e = b[np.where(inside, ty >> 1, 0), np.where(inside, tx >> 1, 0)]
    d = np.where(inside, np.abs(a[..., 0] + e[..., 0]) + np.abs(a[..., 1] + e[..., 1]), 0)
    mask = np.where(inside, (d > tol).astype(np.uint8), 2).astype(np.uint8)
    if window is None:
        window = (0, 0, CW, CH)
    x0, y0, w, h = window
    m, dd = mask[y0:y0 + h, x0:x0 + w], d[y0:y0 + h, x0:x0 + w]
    return mask, (int((m == 0).sum()), int((m == 1).sum()), int((m == 2).sum()), int(dd.sum()))


def small_grids(CH, CW, rng, reach=3):
    """Two random grids of small vectors (most targets inside the plane)."""
    return (rng.integers(-reach, reach + 1, (CH, CW, 2)).astype(np.int16),
            rng.integers(-reach, reach + 1, (CH, CW, 2)).astype(np.int16))


def leaving_grids(CH, CW, rng):
    """Vectors of up to the plane's size: targets leave the plane on every side."""
    a = np.stack([rng.integers(-2 * CW, 2 * CW + 1, (CH, CW)), rng.integers(-2 * CH, 2 * CH + 1, (CH, CW))], -1).astype(np.int16)
    b = np.stack([rng.integers(-2 * CW, 2 * CW + 1, (CH, CW)), rng.integers(-2 * CH, 2 * CH + 1, (CH, CW))], -1).astype(np.int16)
    return a, b


def extreme_grids(CH, CW, rng):
    """Small vectors with the int16 extremes sprinkled into both grids; B carries extremes at the cells A's zero and small
    vectors look at, so that d reaches 131 070 (32767 + 32767 twice) and -32768 + -32768 occurs."""
    a, b = small_grids(CH, CW, rng, 2)
    n = CH * CW
    for k, i in enumerate(rng.choice(n, n // 5, replace=False)):
        b[i // CW, i % CW] = INT16_SPECIALS[k % len(INT16_SPECIALS)]
    for k, i in enumerate(rng.choice(n, n // 8, replace=False)):
        a[i // CW, i % CW] = INT16_SPECIALS[k % len(INT16_SPECIALS)]
    # a pair that is sure to be read: cell (0, 0) stays in place and meets each sum of equal signs
    a[0, 0], b[0, 0] = (32767, 32767), (32767, 32767)          # target outside
    a[1, 1], b[1, 1] = (0, 0), (32767, 32767)
    a[2, 2], b[2, 2] = (1, 1), (32767, 32767)                  # 2 * 32768 = 65 536 = tol 65 535 + 1
    a[3, 3], b[3, 3] = (0, 1), (-32768, -32768)
    return a, b


def windows_of(CH, CW):
    return [None, (0, 0, CW, CH), (CW // 3, CH // 2, 1, 1), (0, CH // 3, CW, 1), (CW - 1, 0, 1, CH),
            (CW - 5, CH - 3, 5, 3), (1, 1, CW - 3, CH - 2)]


GRID_SHAPES = [(24, 32), (26, 38), (17, 30), (40, 6)]           # (CH, CW): CW even, 38 / 30 / 6 not multiples of 4
TOLS = (0, 1, 2, 65535)
GENERATORS = {"small": small_grids, "leaving": leaving_grids, "extreme": extreme_grids}


def host_stats(bbme, a, b, tol, window):
    mask, st = bbme.cells_consistency(a, b, tol, window)
    return mask, tuple(st[k] for k in STAT_KEYS)


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    d, p = C.c_int(), C.c_void_p()
    inv = _capi.ERR_INVALID
    # a null context is refused before anything touches a device
    assert L.bbme_set_direction(None, 0) == inv
    assert L.bbme_get_direction(None, C.byref(d)) == inv
    assert L.bbme_estimate_bidirectional(None) == inv
    assert L.bbme_backward_cells_device_pair(None, 0, C.byref(p)) == inv
    assert L.bbme_get_backward_cells_host_pair(None, 0, buf.ctypes.data) == inv
    assert L.bbme_cells_consistency_device(None, buf.ctypes.data, buf.ctypes.data, 1, None, buf.ctypes.data, 8, st, None) == inv
    assert L.bbme_get_consistency_host(None, 0, 0, 1, buf.ctypes.data) == inv
    assert L.bbme_consistency_stats(None, 0, 1, None, st) == inv
    for name in ("cells_consistency", "DIR_FORWARD", "DIR_BACKWARD", "FB_CONSISTENT", "FB_INCONSISTENT", "FB_OUTSIDE"):
        assert hasattr(bbme, name), name
    for name in ("set_direction", "direction", "estimate_bidirectional_async", "get_backward_cells", "backward_cells_device_ptr",
                 "consistency", "consistency_stats", "cells_consistency_device"):
        assert hasattr(bbme.MF, name), name
    for name in ("get_pair_backward_cells", "consistency_stats_all"):
        assert hasattr(bbme.MFBatch, name), name
    from blockbasedmotionestimation_amd import sequence
    assert hasattr(sequence, "estimate_frames_bidirectional")


@pytest.mark.parametrize("CH,CW", GRID_SHAPES)
@pytest.mark.parametrize("kind", list(GENERATORS))
def test_host_rule_equals_numpy(bbme, kind, CH, CW):
    rng = np.random.default_rng(1000 * CH + CW + len(kind))
    a, b = GENERATORS[kind](CH, CW, rng)
    seen = set()
    for tol in TOLS:
        for window in windows_of(CH, CW):
            exp_mask, exp = np_cells_consistency(a, b, tol, window)
            mask, got = host_stats(bbme, a, b, tol, window)
            assert np.array_equal(mask, exp_mask), (tol, window)
            assert got == exp, (tol, window)
        seen |= set(np.unique(exp_mask).tolist())
    if kind == "leaving":
        m, _ = np_cells_consistency(a, b, 1)
        for ys in (slice(0, 3), slice(CH - 3, CH)):                 # class 2 in every quadrant's border
            for xs in (slice(0, CW // 2), slice(CW // 2, CW)):
                assert (m[ys, xs] == 2).any(), (ys, xs)
        for xs in (slice(0, 3), slice(CW - 3, CW)):
            for ys in (slice(0, CH // 2), slice(CH // 2, CH)):
                assert (m[ys, xs] == 2).any(), (ys, xs)
    if kind == "extreme":
        assert seen == {0, 1, 2}
        _, st = np_cells_consistency(a, b, 65535)
        assert st[1] >= 1                                        # d = 65 536 and 131 070 are beyond the largest tolerance
        m = np_cells_consistency(a, b, 65535)[0]
        assert m[0, 0] == 2
        assert m[1, 1] == 0                                      # |0 + 32767| * 2 = 65 534
        assert m[2, 2] == 1                                      # |1 + 32767| * 2 = 65 536
        assert m[3, 3] == 0                                      # b[3, 3] = (-32768, -32768): 32 768 + 32 767 = 65 535 = tol


def test_sums_beyond_sixteen_bits(bbme):
    """-32768 + -32768 needs a cell whose own vector keeps it inside the plane, i.e. a plane of more than 32 768 pixels in that
    dimension: a = (-32768, -4) from cell (16384, 2) -> pixel (0, 0), b[0, 0] = (-32768, -32768): d = 65 536 + 32 772."""
    CH, CW = 4, 16386
    a = np.zeros((CH, CW, 2), np.int16)
    b = np.zeros((CH, CW, 2), np.int16)
    a[2, 16384] = (-32768, -4)
    b[0, 0] = (-32768, -32768)
    a[3, 16385] = (32767, 0)                           # target x = 65 537 is outside a plane of 32 772 pixels
    win = (16380, 0, 6, 4)
    for tol in (0, 65535):
        mask, st = host_stats(bbme, a, b, tol, win)
        assert st == (22, 1, 1, 98308), tol
        assert mask[2, 16384] == 1 and mask[3, 16385] == 2 and mask[0, 0] == 1 and int(mask.sum()) == 4      # (0, 0) reads b[0, 0] too
        m, s = np_cells_consistency(a, b, tol, win)
        assert np.array_equal(m, mask) and s == st


def test_hand_made_cases(bbme):
    CH, CW = 20, 30
    z = np.zeros((CH, CW, 2), np.int16)
    mask, st = host_stats(bbme, z, z, 0, None)
    assert not mask.any() and st == (CH * CW, 0, 0, 0)
    a = np.empty((CH, CW, 2), np.int16)
    a[...] = (3, -2)
    b = np.empty((CH, CW, 2), np.int16)
    b[...] = (-3, 2)
    # tx = 2 cx + 3 < 60 <=> cx <= 28: the last column leaves on the right; ty = 2 cy - 2 >= 0 <=> cy >= 1: the first row at the top
    outside = CH + CW - 1
    mask, st = host_stats(bbme, a, b, 0, None)
    assert st == (CH * CW - outside, 0, outside, 0)
    assert (mask[0] == 2).all() and (mask[:, -1] == 2).all() and not mask[1:, :-1].any()
    b[...] = (-3, 3)                                                 # d = 1 wherever defined
    mask1, st1 = host_stats(bbme, a, b, 1, None)
    assert st1 == (CH * CW - outside, 0, outside, CH * CW - outside) and np.array_equal(mask1, mask)
    mask0, st0 = host_stats(bbme, a, b, 0, None)
    assert st0 == (0, CH * CW - outside, outside, CH * CW - outside)
    assert (mask0[1:, :-1] == 1).all() and (mask0[0] == 2).all() and (mask0[:, -1] == 2).all()
    # the numpy restatement agrees on all of them
    for tol in (0, 1):
        m, s = np_cells_consistency(a, b, tol)
        assert np.array_equal(m, mask0 if tol == 0 else mask1) and s == (st0 if tol == 0 else st1)


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    CH, CW = 6, 8
    g = np.zeros((CH, CW, 2), np.int16)
    mask = np.zeros((CH, CW), np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID

    def call(a=g.ctypes.data, b=g.ctypes.data, w=CW, h=CH, tol=1, win=None, m=mask.ctypes.data, s=st):
        return L.bbme_cells_consistency_host(a, b, w, h, tol, win, m, s)

    assert call() == 0
    assert call(a=None) == inv
    assert call(b=None) == inv
    assert call(m=None, s=None) == inv                      # nothing asked for
    assert call(m=None) == 0 and call(s=None) == 0
    assert call(tol=-1) == inv
    assert call(w=0) == inv and call(h=0) == inv
    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (CW - 1, 0, 2, 2), (0, CH - 1, 2, 2), (0, 0, CW + 1, CH)):
        assert call(win=(C.c_int * 4)(*win)) == inv, win
    assert call(win=(C.c_int * 4)(CW - 2, CH - 2, 2, 2)) == 0
    with pytest.raises(bbme.BbmeError) as e:
        bbme.cells_consistency(g, g[:, :4], 1)
    assert e.value.status == inv
