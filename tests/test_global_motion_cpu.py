"""The GLOBAL MOTION RULE and the GLOBAL COMPENSATION RULE of include/bbme.h on the CPU: numpy restatements of the histogram, the
moments and the compensation (the GPU tests compare the kernels against the same restatements) against the host mirrors, bit for
bit; the solve against exact rational arithmetic; recovery of known models from synthetic grids; the rule on the oracle's field.

Recovery table (the largest error of the fitted model at the four plane corners, in grid units; tol = 1 px, 4 iterations, affine),
as test_recovery_on_synthetic_grids prints it: 31 of the 32 cases end between 0.000 and 0.250 grid unit with no cell of the
rectangle an inlier.  The one that does not is 256x192, unit 4, zoom 0.03 / rotation -0.02 with the rectangle on 30 % of the cells:
the component-wise median starts on the rectangle, the fit stays there with all 3640 of its cells among its 4024 inliers and ends
34.2 grid units from the truth.  That is the
rule's limit (a joint two-dimensional mode would not start there); the case is printed, not asserted."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

BINS = 2048
WORD_KEYS = ("inliers", "outliers", "excluded", "residual", "sum_x", "sum_y", "sum_xx", "sum_xy", "sum_yy", "sum_dx", "sum_dy",
             "sum_x_dx", "sum_y_dx", "sum_x_dy", "sum_y_dy", "sum_sq")


# ---- the rules restated in numpy ---------------------------------------------------------------------------------------------
def _in_window(shape, window):
    h, w = shape
    inside = np.zeros((h, w), bool)
    x0, y0, ww, wh = (0, 0, w, h) if window is None else window
    inside[y0:y0 + wh, x0:x0 + ww] = True
    return inside


def np_histogram(cells, exclude=None, window=None):
    cells = np.asarray(cells, np.int16)
    use = _in_window(cells.shape[:2], window)
    if exclude is not None:
        use &= np.asarray(exclude) == 0
    out = np.zeros((2, BINS), np.uint32)
    for k in range(2):
        out[k] = np.bincount(np.clip(cells[..., k][use].astype(np.int64), -1024, 1023) + 1024, minlength=BINS)
    return out


def np_median(hist_row):
    n = int(hist_row.sum())
    if n == 0:
        return 0
    return int(np.searchsorted(np.cumsum(hist_row.astype(np.int64)), (n + 1) >> 1)) - 1024


def cell_coordinates(ch, cw):
    """X (1, CW) and Y (CH, 1): half pixels from the plane centre."""
    return (4 * np.arange(cw, dtype=np.int64) + 2 - 2 * cw)[None, :], (4 * np.arange(ch, dtype=np.int64) + 2 - 2 * ch)[:, None]


def np_moments(cells, model, tol, exclude=None, window=None):
    cells = np.asarray(cells, np.int16)
    ch, cw = cells.shape[:2]
    m = [int(v) for v in model]
    X, Y = cell_coordinates(ch, cw)
    X, Y = np.broadcast_to(X, (ch, cw)), np.broadcast_to(Y, (ch, cw))
    dx, dy = cells[..., 0].astype(np.int64), cells[..., 1].astype(np.int64)
    r = np.abs(dx * 65536 - (m[0] + m[1] * X + m[2] * Y)) + np.abs(dy * 65536 - (m[3] + m[4] * X + m[5] * Y))
    cls = np.where(r <= tol, 0, 1).astype(np.uint8)
    if exclude is not None:
        cls[np.asarray(exclude) != 0] = 2
    win = _in_window((ch, cw), window)
    inl = win & (cls == 0)
    terms = (r, X, Y, X * X, X * Y, Y * Y, dx, dy, X * dx, Y * dx, X * dy, Y * dy, dx * dx + dy * dy)
    words = [int((win & (cls == k)).sum()) for k in range(3)] + [int(t[inl].sum(dtype=np.int64)) for t in terms]
    return cls, np.array(words, np.int64)


def np_estimate(bbme, cells, kind, tol, iterations, exclude=None, window=None):
    """Part 4 of the rule with the numpy parts and the library's solve."""
    hist = np_histogram(cells, exclude, window)
    model = np.zeros(6, np.int32)
    if hist[0].sum():
        model[0], model[3] = np_median(hist[0]) << 16, np_median(hist[1]) << 16
        for _ in range(iterations):
            _, w = np_moments(cells, model, tol, exclude, window)
            if w[0] == 0:
                break
            model = bbme.solve_global_motion(w, kind)
    cls, words = np_moments(cells, model, tol, exclude, window)
    return model, words, cls


def np_global_compensate(I1, I2, model, unit=1, fill=0, window=None):
    I2 = np.asarray(I2, np.uint8)
    h, w = I2.shape
    m = [int(v) for v in model]
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    X, Y = 2 * x + 1 - w, 2 * y + 1 - h
    mul = 4 // unit
    qx = ((m[0] + m[1] * X + m[2] * Y) * mul + 32768) >> 16
    qy = ((m[3] + m[4] * X + m[5] * Y) * mul + 32768) >> 16
    fx, fy = qx & 3, qy & 3
    sx, sy = x + (qx >> 2), y + (qy >> 2)
    x1, y1 = (fx != 0).astype(np.int64), (fy != 0).astype(np.int64)
    ok = (sx >= 0) & (sx + 1 + x1 <= w) & (sy >= 0) & (sy + 1 + y1 <= h)
    cx, cy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)                # a tap of weight 0 folds onto the first
    cx1, cy1 = np.clip(sx + x1, 0, w - 1), np.clip(sy + y1, 0, h - 1)
    P = I2.astype(np.int64)
    v = ((4 - fx) * (4 - fy) * P[cy, cx] + fx * (4 - fy) * P[cy, cx1] + (4 - fx) * fy * P[cy1, cx] + fx * fy * P[cy1, cx1] + 8) >> 4
    out = np.where(ok, v, fill).astype(np.uint8)
    stats = None
    if I1 is not None:
        win = _in_window((h, w), window)
        d = v - np.asarray(I1, np.int64)
        sel = win & ok
        stats = (int((d * d)[sel].sum()), int(np.abs(d)[sel].sum()), int(sel.sum()), int((win & ~ok).sum()))
    return out, stats


STAT_KEYS = ("sse", "sad", "pixels", "skipped")


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def random_grid(ch, cw, seed, spread=6):
    return np.random.default_rng(seed).integers(-spread, spread + 1, size=(ch, cw, 2)).astype(np.int16)


def extreme_grid(ch, cw, seed):
    """int16 extremes and values on and around both ends of the bins among small vectors"""
    rng = np.random.default_rng(seed)
    g = rng.integers(-3, 4, size=(ch, cw, 2)).astype(np.int16)
    special = np.array([-32768, 32767, -1025, -1024, -1023, 1022, 1023, 1024, 0], np.int16)
    pick = rng.random((ch, cw, 2)) < 0.3
    g[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    return g


def uniform_grid(ch, cw, v=(3, -2)):
    g = np.empty((ch, cw, 2), np.int16)
    g[...] = v
    return g


def cutting_windows(cw, ch):
    """windows in cells that start and end inside runs of 4, one cell, the last column, everything"""
    return [(1, 1, cw - 3, ch - 2), (3, 0, 2, ch), (cw - 1, 0, 1, ch), (0, ch - 1, cw, 1), (2, 3, 1, 1), (0, 0, cw, ch)]


def random_mask(ch, cw, seed, p=0.3):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 256, size=(ch, cw)) * (rng.random((ch, cw)) < p)).astype(np.uint8)


MODELS = [
    (0, 0, 0, 0, 0, 0),
    (3 << 16, 0, 0, -(2 << 16), 0, 0),
    (212992, 655, -328, -98304, 328, 655),
    (2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1, -2 ** 31),
    (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1),
]
TOLS = [0, 65536, 3 * 65536, 2 ** 40]
GRID_SHAPES = [(10, 18), (25, 33), (48, 64)]


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    for name in ("bbme_vector_histogram_host", "bbme_global_moments_host", "bbme_global_motion_solve_host", "bbme_global_motion_host",
                 "bbme_global_compensate_host", "bbme_cells_vector_histogram_device", "bbme_cells_global_moments_device",
                 "bbme_cells_global_compensate_device", "bbme_global_motion", "bbme_get_global_motion_map_host",
                 "bbme_global_compensate_device", "bbme_get_global_compensated_host", "bbme_global_compensation_error"):
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    for name in ("global_motion", "draw_MVimage_global", "compensation_error_global", "cells_vector_histogram_device",
                 "cells_global_moments_device", "cells_global_compensate_device"):
        assert hasattr(bbme.MF, name), name
    assert hasattr(bbme.MFBatch, "global_motion_all") and hasattr(bbme.MFChain, "global_motion_all")


@pytest.mark.parametrize("ch,cw", GRID_SHAPES)
def test_histogram_host_equals_numpy(bbme, ch, cw):
    for name, g in (("random", random_grid(ch, cw, 1)), ("extreme", extreme_grid(ch, cw, 2)), ("uniform", uniform_grid(ch, cw))):
        mask = random_mask(ch, cw, 3)
        wide = np.full((ch, cw + 3), 255, np.uint8)
        wide[:, :cw] = mask
        for window in [None] + cutting_windows(cw, ch):
            for excl in (None, mask, wide[:, :cw]):
                got = bbme.vector_histogram_cells(g, excl, window)
                exp = np_histogram(g, excl, window)
                assert np.array_equal(got, exp), (name, window, excl is not None)
        if name == "extreme":
            h = bbme.vector_histogram_cells(g)
            assert h[0, 0] > 0 and h[0, BINS - 1] > 0 and h[1, 0] > 0 and h[1, BINS - 1] > 0      # the end bins
    # n = 0: every cell excluded
    assert bbme.vector_histogram_cells(random_grid(ch, cw, 4), np.ones((ch, cw), np.uint8)).sum() == 0


@pytest.mark.parametrize("ch,cw", GRID_SHAPES)
def test_moments_host_equals_numpy(bbme, ch, cw):
    grids = (("random", random_grid(ch, cw, 5)), ("extreme", extreme_grid(ch, cw, 6)), ("uniform", uniform_grid(ch, cw)))
    mask = random_mask(ch, cw, 7)
    seen_inliers = seen_none = False
    for name, g in grids:
        for model in MODELS:
            for tol in TOLS:
                for window in (None, cutting_windows(cw, ch)[0], cutting_windows(cw, ch)[4]):
                    for excl in (None, mask):
                        got_map, got = bbme.global_moments_cells(g, model, tol, excl, window)
                        exp_map, exp = np_moments(g, model, tol, excl, window)
                        assert np.array_equal(got_map, exp_map), (name, model, tol, window)
                        assert np.array_equal(got, exp), (name, model, tol, window, dict(zip(WORD_KEYS, zip(got, exp))))
                        assert got[0] + got[1] + got[2] == (window[2] * window[3] if window else ch * cw)
                        seen_inliers |= got[0] > 0
                        seen_none |= got[0] == 0                  # n0 = 0
    assert seen_inliers and seen_none
    # every cell excluded: n2 alone
    _, w = bbme.global_moments_cells(grids[0][1], MODELS[1], 65536, np.full((ch, cw), 7, np.uint8))
    assert w.tolist() == [0, 0, ch * cw] + [0] * 13


def test_estimate_host_equals_numpy_parts(bbme):
    """bbme_global_motion_host is Part 4 made of the parts"""
    for ch, cw in GRID_SHAPES:
        mask = random_mask(ch, cw, 8)
        for name, g in (("random", random_grid(ch, cw, 9, 2)), ("extreme", extreme_grid(ch, cw, 10)), ("uniform", uniform_grid(ch, cw))):
            for kind in ("translation", "affine"):
                for tol in (0, 65536, 2 ** 40):
                    for iterations in (0, 1, 4, 8):
                        for excl, window in ((None, None), (mask, cutting_windows(cw, ch)[0])):
                            got = bbme.global_motion_cells(g, kind, tol, iterations, excl, window)
                            exp = np_estimate(bbme, g, kind, tol, iterations, excl, window)
                            for a, b, what in zip(got, exp, ("model", "words", "map")):
                                assert np.array_equal(a, b), (name, kind, tol, iterations, what, a, b)
        # n = 0
        model, words, cls = bbme.global_motion_cells(random_grid(ch, cw, 11), "affine", 65536, 3, np.ones((ch, cw), np.uint8))
        assert not model.any() and words.tolist() == [0, 0, ch * cw] + [0] * 13 and (cls == 2).all()
    # the uniform grid is found exactly, with every cell an inlier, at tol 0
    model, words, cls = bbme.global_motion_cells(uniform_grid(20, 30, (5, -7)), "affine", 0, 2)
    assert model.tolist() == [5 << 16, 0, 0, -(7 << 16), 0, 0] and words[0] == 600 and words[3] == 0 and not cls.any()


# ---- the solve against exact rational arithmetic -----------------------------------------------------------------------------
def fraction_solve(w):
    """The exactly rounded least-squares solution of the normal equations: six Q16 integers"""
    n, sx, sy, sxx, sxy, syy = (int(w[k]) for k in (0, 4, 5, 6, 7, 8))
    A = [[n, sx, sy], [sx, sxx, sxy], [sy, sxy, syy]]

    def det(M):
        return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
                + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))
    D = det(A)
    out = []
    for rhs in ([int(w[9]), int(w[11]), int(w[12])], [int(w[10]), int(w[13]), int(w[14])]):
        for k in range(3):
            M = [row[:] for row in A]
            for i in range(3):
                M[i][k] = rhs[i]
            out.append(round(Fraction(det(M), D) * 65536))            # round() of a Fraction is half to even
    return out


def affine_cells(ch, cw, unit, tx, ty, zoom, rot):
    """rint of the true affine field in grid units, and the true model as six floats (grid units, per half pixel)"""
    X, Y = cell_coordinates(ch, cw)
    true = np.array([unit * tx, unit * zoom / 2, -unit * rot / 2, unit * ty, unit * rot / 2, unit * zoom / 2])
    g = np.empty((ch, cw, 2), np.int16)
    g[..., 0] = np.rint(true[0] + true[1] * X + true[2] * Y)
    g[..., 1] = np.rint(true[3] + true[4] * X + true[5] * Y)
    return g, true


PROTOTYPE_PLANES = [(36, 20), (128, 96), (4096, 2304), (8188, 8188)]


@pytest.mark.parametrize("w,h", PROTOTYPE_PLANES)
def test_solve_equals_the_exact_rational_solution(bbme, w, h):
    ch, cw = h // 2, w // 2
    zoom, rot = (0.001, -0.0007) if w > 4000 else (0.02, -0.015)       # the vectors stay inside int16 on the large planes
    g, _ = affine_cells(ch, cw, 4, 3.25, -1.5, zoom, rot)
    rng = np.random.default_rng(w)
    g += rng.integers(-2, 3, size=g.shape).astype(np.int16)
    strip = np.ones((ch, cw), np.uint8)
    strip[ch // 3:ch // 3 + 2, :] = 0
    selections = (("full", None), ("30 % random", (rng.random((ch, cw)) >= 0.3).astype(np.uint8)), ("thin strip", strip))
    for name, excl in selections:
        _, words = bbme.global_moments_cells(g, (0,) * 6, 2 ** 40, excl)          # every selected cell an inlier
        assert words[0] == (ch * cw if excl is None else int((excl == 0).sum())) and words[1] == 0
        assert all(abs(int(v)) < 2 ** 53 for v in words)
        got = bbme.solve_global_motion(words, "affine").tolist()
        exact = fraction_solve(words)
        assert got[1] != 0 and got[5] != 0, (name, got)                           # not the fallback
        assert max(abs(a - b) for a, b in zip(got, exact)) <= 1, (name, got, exact)
        t = bbme.solve_global_motion(words, "translation").tolist()
        assert t == [round(Fraction(int(words[9]), int(words[0])) * 65536), 0, 0,
                     round(Fraction(int(words[10]), int(words[0])) * 65536), 0, 0], name


def test_solve_falls_back_to_the_translation(bbme):
    ch, cw = 24, 40
    g, _ = affine_cells(ch, cw, 1, 3.0, -2.0, 0.05, 0.03)
    two = np.ones((ch, cw), np.uint8)
    two[3, 4] = two[17, 30] = 0
    column = np.ones((ch, cw), np.uint8)
    column[:, 7] = 0
    diagonal = np.ones((ch, cw), np.uint8)
    diagonal[np.arange(ch), np.arange(ch)] = 0
    for name, excl in (("n0 < 3", two), ("one column", column), ("a diagonal line", diagonal)):
        _, words = bbme.global_moments_cells(g, (0,) * 6, 2 ** 40, excl)
        assert words[0] == int((excl == 0).sum())
        got = bbme.solve_global_motion(words, "affine").tolist()
        assert got == bbme.solve_global_motion(words, "translation").tolist(), name
        assert got[1] == got[2] == got[4] == got[5] == 0 and got[0] == round(Fraction(int(words[9]), int(words[0])) * 65536), name
    # n0 = 0: the zero model; three cells that span the plane: affine
    assert bbme.solve_global_motion([0] * 16, "affine").tolist() == [0] * 6
    three = np.ones((ch, cw), np.uint8)
    three[0, 0] = three[0, cw - 1] = three[ch - 1, 0] = 0
    _, words = bbme.global_moments_cells(g, (0,) * 6, 2 ** 40, three)
    assert bbme.solve_global_motion(words, "affine")[1] != 0
    for bad in (dict(kind=2), dict(kind=-1)):
        from blockbasedmotionestimation_amd import _capi
        m = np.zeros(6, np.int32)
        assert _capi.lib().bbme_global_motion_solve_host(words.ctypes.data, bad["kind"], m.ctypes.data) == -1


# ---- recovery of a known model -------------------------------------------------------------------------------------------------
MOTIONS = [(0.0, 0.0), (0.02, 0.0), (0.0, 0.02), (0.03, -0.02)]          # (zoom per pixel, rotation)
RECOVERY = [(w, h, unit, zoom, rot, share) for (w, h) in ((128, 96), (256, 192)) for unit in (1, 4) for zoom, rot in MOTIONS
            for share in (0, 30)]
THE_LIMIT = (256, 192, 4, 0.03, -0.02, 30)


def recovery_case(bbme, w, h, unit, zoom, rot, share):
    ch, cw = h // 2, w // 2
    g, true = affine_cells(ch, cw, unit, 3.25, -1.75 if unit == 1 else -1.5, zoom, rot)
    rect = np.zeros((ch, cw), bool)
    if share:
        rw, rh = int(0.55 * cw), int(0.55 * ch)                           # 30 % of the cells
        rect[ch // 8:ch // 8 + rh, cw // 8:cw // 8 + rw] = True
        g[rect] = (24, -8)
    model, words, cls = bbme.global_motion_cells(g, "affine", unit * 65536, 4)
    m = model / 65536.0
    err = max(max(abs((m[0] + m[1] * X + m[2] * Y) - (true[0] + true[1] * X + true[2] * Y)),
                  abs((m[3] + m[4] * X + m[5] * Y) - (true[3] + true[4] * X + true[5] * Y))) for X in (-w, w) for Y in (-h, h))
    return err, int((cls[rect] == 0).sum()), int(rect.sum()), words


def test_recovery_on_synthetic_grids(bbme):
    failures = []
    print()
    for case in RECOVERY:
        err, rect_inliers, rect_cells, words = recovery_case(bbme, *case)
        print("%4dx%-4d unit %d zoom %.2f rot %+.2f rect %2d %%: corner error %8.3f grid units, %5d of %5d rectangle cells inliers, "
              "%5d inliers%s" % (case + (err, rect_inliers, rect_cells, int(words[0]), "   <- the rule's limit" if case == THE_LIMIT else "")))
        if case != THE_LIMIT and not (err <= 0.5 and rect_inliers == 0):
            failures.append((case, err, rect_inliers))
    assert not failures, failures


# ---- the rule on the oracle's field --------------------------------------------------------------------------------------------
def test_pipeline_on_the_oracles_field(bbme, oracle):
    """A pair cut from one texture at an integer offset, a pasted block (about 20 % of the area) moving differently"""
    rng = np.random.default_rng(77)
    w, h, off, block_off = 128, 96, (3, -2), (-4, 3)
    big = rng.integers(0, 256, size=(h + 32, w + 32)).astype(np.float64)
    for _ in range(2):                                                    # a texture smooth enough to match
        big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) / 4
    big = np.clip((big - big.mean()) * 3 + 128, 0, 255).astype(np.uint8)
    f1 = big[16:16 + h, 16:16 + w].copy()
    f2 = big[16 + off[1]:16 + off[1] + h, 16 + off[0]:16 + off[0] + w].copy()        # f1[y][x] = f2[y - off.y][x - off.x]
    patch = rng.integers(0, 256, size=(44, 56)).astype(np.uint8)         # 44 x 56 of 96 x 128: 20 %
    bx, by = 40, 28
    f1[by:by + 44, bx:bx + 56] = patch
    f2[by + block_off[1]:by + block_off[1] + 44, bx + block_off[0]:bx + block_off[0] + 56] = patch
    mf = oracle.OracleMF(f1, f2, [16, 16], [8, 8])
    flow = mf.calc_motion_block_matching()
    cells = np.ascontiguousarray(flow[::2, ::2]).astype(np.int16)
    px, py = mf.padding_x, mf.padding_y
    window = (-(-px // 2), -(-py // 2), w // 2, h // 2)
    model, words, cls = bbme.global_motion_cells(cells, "translation", 65536, 3, None, window)
    assert (int(np.rint(model[0] / 65536)), int(np.rint(model[3] / 65536))) == (-off[0], -off[1]), (model, words)
    assert not model[[1, 2, 4, 5]].any()
    interior = cls[(py + by + 8) // 2:(py + by + 36) // 2, (px + bx + 8) // 2:(px + bx + 48) // 2]
    assert (interior == 1).all(), interior
    assert words[0] > 0.6 * window[2] * window[3]
    mf.close()


# ---- global compensation -------------------------------------------------------------------------------------------------------
def plane_windows(w, h):
    return [(1, 1, w - 3, h - 2), (3, 0, 2, h), (w - 1, h - 1, 1, 1), (0, 0, w, h)]


COMP_MODELS = [((212992, 655, -328, -98304, 328, 655), 1), ((851968, 2621, -1310, -393216, 1310, 2621), 4),
               ((0, 40000, 0, 0, 0, -40000), 1), ((12345, -7, 3, -54321, 2, 9), 4), ((2 ** 31 - 1, 0, 0, 0, 0, 0), 1),
               ((0, 0, 0, -2 ** 31, 0, 0), 4), ((2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1, -2 ** 31), 1)]


@pytest.mark.parametrize("w,h", [(36, 20), (70, 50)])
def test_compensation_host_equals_numpy(bbme, w, h):
    rng = np.random.default_rng(w)
    I1, I2 = rng.integers(0, 256, size=(2, h, w)).astype(np.uint8)
    skipped_all = 0
    for model, unit in COMP_MODELS:
        for fill, window in zip((0, 7, 255, 128, 0), [None] + plane_windows(w, h)):
            out, st = bbme.global_compensate(I1, I2, model, unit, fill, window)
            exp_out, exp_st = np_global_compensate(I1, I2, model, unit, fill, window)
            assert np.array_equal(out, exp_out), (model, unit, fill)
            assert tuple(st[k] for k in STAT_KEYS) == exp_st, (model, unit, window)
            skipped_all += exp_st[2] == 0                              # models that skip everything
    assert skipped_all >= 10
    # the statistics do not depend on fill; the frame without image 1
    a = bbme.global_compensate(I1, I2, COMP_MODELS[0][0], 1, 0)[1]
    b = bbme.global_compensate(I1, I2, COMP_MODELS[0][0], 1, 200)[1]
    assert a == b
    out, st = bbme.global_compensate(None, I2, COMP_MODELS[0][0], 1, 9)
    assert st is None and np.array_equal(out, np_global_compensate(None, I2, COMP_MODELS[0][0], 1, 9)[0])


def test_whole_pixel_translation_property(bbme):
    rng = np.random.default_rng(5)
    h, w = 40, 56
    I2 = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    for unit in (1, 4):
        for tx, ty in ((0, 0), (3, -2), (-7, 5), (w, 0), (-1, h - 1)):
            out, st = bbme.global_compensate(I2, I2, (tx * unit << 16, 0, 0, ty * unit << 16, 0, 0), unit, 77)
            exp = np.full((h, w), 77, np.uint8)
            ys, xs = np.mgrid[0:h, 0:w]
            ok = (ys + ty >= 0) & (ys + ty < h) & (xs + tx >= 0) & (xs + tx < w)
            exp[ok] = I2[(ys + ty)[ok], (xs + tx)[ok]]
            assert np.array_equal(out, exp), (unit, tx, ty)
            assert st["pixels"] == int(ok.sum()) and st["skipped"] == h * w - int(ok.sum())


def test_host_rules_refuse_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    g = random_grid(8, 10, 1)
    hist = np.zeros((2, BINS), np.uint32)
    words = np.zeros(16, np.int64)
    model = np.zeros(6, np.int32)
    cls = np.zeros((8, 10), np.uint8)
    I = np.zeros((16, 20), np.uint8)
    st = (C.c_ulonglong * 4)()
    win = lambda *v: (C.c_int * 4)(*v)                                    # noqa: E731
    bad = [
        lib.bbme_vector_histogram_host(None, 10, 8, None, 0, None, hist.ctypes.data),
        lib.bbme_vector_histogram_host(g.ctypes.data, 10, 8, None, 0, None, None),
        lib.bbme_vector_histogram_host(g.ctypes.data, 0, 8, None, 0, None, hist.ctypes.data),
        lib.bbme_vector_histogram_host(g.ctypes.data, 10, 8, cls.ctypes.data, 9, None, hist.ctypes.data),
        lib.bbme_vector_histogram_host(g.ctypes.data, 10, 8, None, 0, win(0, 0, 11, 1), hist.ctypes.data),
        lib.bbme_vector_histogram_host(g.ctypes.data, 10, 8, None, 0, win(-1, 0, 2, 1), hist.ctypes.data),
        lib.bbme_global_moments_host(g.ctypes.data, 10, 8, None, 0, model.ctypes.data, 0, None, None, None),
        lib.bbme_global_moments_host(g.ctypes.data, 10, 8, None, 0, None, 0, None, cls.ctypes.data, words.ctypes.data),
        lib.bbme_global_moments_host(g.ctypes.data, 10, 8, None, 0, model.ctypes.data, -1, None, cls.ctypes.data, None),
        lib.bbme_global_moments_host(g.ctypes.data, 10, 8, None, 0, model.ctypes.data, 2 ** 40 + 1, None, cls.ctypes.data, None),
        lib.bbme_global_motion_host(g.ctypes.data, 10, 8, None, 0, 1, 65536, 9, None, model.ctypes.data, None, None),
        lib.bbme_global_motion_host(g.ctypes.data, 10, 8, None, 0, 1, 65536, -1, None, model.ctypes.data, None, None),
        lib.bbme_global_motion_host(g.ctypes.data, 10, 8, None, 0, 2, 65536, 1, None, model.ctypes.data, None, None),
        lib.bbme_global_motion_host(g.ctypes.data, 10, 8, None, 0, 1, 65536, 1, None, None, None, None),
        lib.bbme_global_compensate_host(I.ctypes.data, I.ctypes.data, 20, 16, model.ctypes.data, 2, 0, None, cls.ctypes.data, None),
        lib.bbme_global_compensate_host(I.ctypes.data, I.ctypes.data, 20, 16, model.ctypes.data, 1, 256, None, cls.ctypes.data, None),
        lib.bbme_global_compensate_host(I.ctypes.data, I.ctypes.data, 19, 16, model.ctypes.data, 1, 0, None, cls.ctypes.data, None),
        lib.bbme_global_compensate_host(None, I.ctypes.data, 20, 16, model.ctypes.data, 1, 0, None, None, st),
        lib.bbme_global_compensate_host(I.ctypes.data, I.ctypes.data, 20, 16, model.ctypes.data, 1, 0, None, None, None),
        lib.bbme_global_compensate_host(I.ctypes.data, I.ctypes.data, 20, 16, model.ctypes.data, 1, 0, win(0, 0, 21, 1), None, st),
    ]
    assert bad == [-1] * len(bad), bad
    assert lib.bbme_vector_histogram_host(g.ctypes.data, 4095, 8, None, 0, None, hist.ctypes.data) == -8
    assert lib.bbme_global_compensate_host(None, I.ctypes.data, 8190, 16, model.ctypes.data, 1, 0, None, cls.ctypes.data, None) == -8
    # the estimate alone, without words or map
    assert lib.bbme_global_motion_host(g.ctypes.data, 10, 8, None, 0, 1, 65536, 2, None, model.ctypes.data, None, None) == 0
