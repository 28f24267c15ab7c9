"""CPU tests of the subpel temporal filter rule (include/bbme.h, "SUBPEL TEMPORAL FILTER RULE"): the C-ABI exports the calls;
bbme_subpel_temporal_filter_host follows the rule, which is restated here in vectorised numpy from the header's text and imported
by the GPU tests; the rule's three properties, validity at every plane edge and every quotient of the two divisions -- on plane
bytes and on rounded bilinear samples -- carry their answers written out; on noisy frames of sub-pixel motion the filtered middle
frame gains what the integer rule cannot."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from test_gpu_bidirectional import _oracle_fields
from test_interpolation_cpu import extreme_grids, odd_windows, psnr, random_grids
from test_subpel_interpolation_cpu import _motion_field, fraction_grids, frames_of, hires_texture
from test_temporal_filter_cpu import (RULE_THRS, S23_THR, STAT_KEYS, THRS, neighbour_sets, np_temporal_filter, s23_table_planes,
                                      s_table_check, s_table_planes, thr_table_expected, thr_table_planes)

NEW_SYMBOLS = ["bbme_subpel_temporal_filter_host", "bbme_cells_subpel_temporal_filter_device", "bbme_subpel_temporal_filter_device",
               "bbme_subpel_temporal_filter_chain_device", "bbme_get_subpel_temporal_filtered_host",
               "bbme_subpel_temporal_filter_stats"]

PLANES = [(16, 16), (20, 24), (28, 36)]                     # (H0, W0); W0 = 36 is 4 mod 8: 18 cells, the last run of a row is cut


def np_subpel_temporal_filter(Cur, P, QP, N, QN, thr, window=None):
    """The rule of include/bbme.h: output cell (cx, cy) with origin o = (2 cx, 2 cy) looks, for each present neighbour X (P with QP,
    N with QN), at (qx, qy) = Q[cy, cx]: s = o + (qx >> 2, qy >> 2), f = (qx & 3, qy & 3); valid when 0 <= s.x, s.x + 2 + (fx != 0)
    <= W0, 0 <= s.y, s.y + 2 + (fy != 0) <= H0; X'[k, j] = ((4 - fx)(4 - fy) X[s + (j, k)] + fx (4 - fy) X[s + (j + 1, k)] +
    (4 - fx) fy X[s + (j, k + 1)] + fx fy X[s + (j + 1, k + 1)] + 8) >> 4; cost = sum |C - X'|; w = 8 (thr - cost) // thr when valid
    and cost < thr, else 0; S = 8 + wP + wN and out = (8 C + wP P' + wN N' + S // 2) // S.  Returns (out, map, statistics) as
    test_temporal_filter_cpu.np_temporal_filter does."""
    Cur = np.asarray(Cur).astype(np.int64)
    H0, W0 = Cur.shape
    CH, CW = H0 // 2, W0 // 2
    assert (P is None) == (QP is None) and (N is None) == (QN is None) and (P is not None or N is not None)
    cy, cx = np.mgrid[0:CH, 0:CW]
    ox, oy = 2 * cx, 2 * cy
    cell = np.stack([np.stack([Cur[oy + k, ox + j] for j in range(2)]) for k in range(2)])      # [k, j, cy, cx]
    ws, moved = [], []
    for X, Q in ((P, QP), (N, QN)):
        if X is None:
            ws.append(np.zeros((CH, CW), np.int64))
            moved.append(np.zeros((2, 2, CH, CW), np.int64))
            continue
        X = np.asarray(X).astype(np.int64)
        Q = np.asarray(Q).astype(np.int64)
        qx, qy = Q[..., 0], Q[..., 1]
        fx, fy = qx & 3, qy & 3
        sx, sy = ox + (qx >> 2), oy + (qy >> 2)
        valid = (sx >= 0) & (sx + 2 + (fx != 0) <= W0) & (sy >= 0) & (sy + 2 + (fy != 0) <= H0)
        sx, sy = np.where(valid, sx, 0), np.where(valid, sy, 0)

        def tap(dx, dy, weight):                            # a tap of weight 0 is not read: its index is folded into the plane
            x = np.where(weight > 0, sx + dx, 0)
            y = np.where(weight > 0, sy + dy, 0)
            return weight * X[np.where(valid, y, 0), np.where(valid, x, 0)]

        m = np.stack([np.stack([(tap(j, k, (4 - fx) * (4 - fy)) + tap(j + 1, k, fx * (4 - fy)) + tap(j, k + 1, (4 - fx) * fy) +
                                 tap(j + 1, k + 1, fx * fy) + 8) >> 4 for j in range(2)]) for k in range(2)])
        cost = np.abs(cell - m).sum(axis=(0, 1))
        ws.append(np.where(valid & (cost < thr), 8 * (thr - cost) // thr, 0))
        moved.append(m)
    wP, wN = ws
    S = 8 + wP + wN
    pix = (8 * cell + wP * moved[0] + wN * moved[1] + S // 2) // S
    out = np.empty((H0, W0), np.uint8)
    for k in range(2):
        for j in range(2):
            out[k::2, j::2] = pix[k, j]
    change = np.abs(pix - cell).sum(axis=(0, 1))
    x0, y0, w, h = (0, 0, CW, CH) if window is None else window
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    stats = (int((wP[sl] > 0).sum()), int((wN[sl] > 0).sum()), int((wP[sl] + wN[sl]).sum()), int(change[sl].sum()))
    return out, (wP | wN << 4).astype(np.uint8), stats


def host(bbme, Cur, P, QP, N, QN, thr, window=None):
    out, wmap, st = bbme.temporal_filter_cells_subpel(Cur, P, N, QP, QN, thr, window)
    return out, wmap, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, Cur, P, QP, N, QN, thr, window=None, what=None):
    exp = np_subpel_temporal_filter(Cur, P, QP, N, QN, thr, window)
    got = host(bbme, Cur, P, QP, N, QN, thr, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert np.array_equal(got[0], exp[0]), tag
    assert np.array_equal(got[1], exp[1]), tag
    assert got[2] == exp[2], tag
    return exp


def near_frames(H0, W0, seed):
    """A smooth plane and two neighbours near it, so that sampled cells pass at the strengths used"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H0, 0:W0]
    Cur = (96 + 5 * x + 3 * y + rng.integers(-6, 7, (H0, W0))).astype(np.int64) % 256
    P = np.clip(Cur + rng.integers(-5, 6, (H0, W0)), 0, 255)
    N = np.clip(Cur + rng.integers(-9, 10, (H0, W0)), 0, 255)
    return Cur.astype(np.uint8), P.astype(np.uint8), N.astype(np.uint8)


def fractions_taken(wmap, QP, QN):
    """The (fx, fy) classes of the cells that took their previous / their next neighbour"""
    return ({(int(a) & 3, int(b) & 3) for a, b in QP[(wmap & 0x0f) > 0]}, {(int(a) & 3, int(b) & 3) for a, b in QN[(wmap >> 4) > 0]})


def inside_axis(p, n):
    """Every tap of non-zero weight of a cell at quarter-pel position p lies in 0 .. n - 1: the header's inequality, on scalars"""
    return 0 <= (p >> 2) and (p >> 2) + 2 + ((p & 3) != 0) <= n


def edge_grid(H0, W0):
    """A quarter-pel grid in which, for each plane edge and each fraction, one cell's s lands on the last valid position with that
    fraction and another one a pixel further out; from the f = 0 extremes also one a QUARTER pel further out.  The other component
    of these cells is 0, every other cell is zero -> (grid, [(cx, cy, valid)]) with `valid` from inside_axis."""
    CH, CW = H0 // 2, W0 // 2
    Q = np.zeros((CH, CW, 2), np.int64)
    cells, used = [], set()
    for axis, (n, cn, co) in enumerate(((W0, CW, CH), (H0, CH, CW))):
        wants = [0, -1, 4 * (n - 2), 4 * (n - 2) + 1]                             # f = 0: on the edge, a quarter pel out
        for f in (1, 2, 3):
            wants += [f, f - 4, 4 * (n - 3) + f, 4 * (n - 2) + f]                 # f != 0: the last position inside, a pixel out
        for k, want in enumerate(wants):
            for t in range(cn * co):
                c, other = (5 * k + t) % cn, (3 * k + 1 + t // cn) % co
                cx, cy = (c, other) if axis == 0 else (other, c)
                if (cx, cy) not in used:
                    break
            used.add((cx, cy))
            Q[cy, cx, axis] = want - 8 * c
            cells.append((cx, cy, inside_axis(want, n)))
    assert np.abs(Q).max() < 32768
    return Q.astype(np.int16), cells


def sampled_cost_table():
    """C = 0 and a neighbour plane of 128 x 64 pixels which, read with the half-pel grid (2, 0), gives the cell in column 2 i of
    cell row r -- table entry k = 32 r + i, k <= 1020 -- four ROUNDED samples that sum to cost k: with q, r4 = divmod(k, 4) the
    samples are (q, q + (r4 > 0); q + (r4 > 2), q + (r4 > 1)), the taps (a, a, b) of a row giving (a + a + 1) >> 1 = a and
    (a + b + 1) >> 1 = b for b = a or a + 1 -- a truncating sample would give a, and another cost.  The odd columns' cells read
    what the even ones left.  Returns (C, X, grid, cost (32, 32) of the table cells)."""
    CH, CW = 32, 64
    X = np.zeros((2 * CH, 2 * CW), np.uint8)
    k = np.minimum(np.arange(32 * 32), 1020).reshape(32, 32)
    q, r4 = k // 4, k % 4
    top = (q, q + (r4 > 0))
    bot = (q + (r4 > 2), q + (r4 > 1))
    for row, (a, b) in enumerate((top, bot)):
        X[row::2, 0::4], X[row::2, 1::4], X[row::2, 2::4] = a, a, b
    grid = np.zeros((CH, CW, 2), np.int16)
    grid[..., 0] = 2
    return np.zeros_like(X), X, grid, k


def sampled_cost_check(k, thr, out, w):
    """The weights of the table cells are the exact quotients and their pixels the blend of the rounded samples with C = 0"""
    exp = thr_table_expected(k, thr)
    assert np.array_equal(w[:, 0::2], exp), thr
    q, r4 = k // 4, k % 4
    samples = ((q, q + (r4 > 0)), (q + (r4 > 2), q + (r4 > 1)))
    S = 8 + exp
    for i in range(2):
        for j in range(2):
            assert np.array_equal(out[i::2, j::4], (exp * samples[i][j] + S // 2) // S), (thr, i, j)
    assert set(k.ravel().tolist()) == set(range(1021))                          # every cost occurs


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
    assert "SUBPEL TEMPORAL FILTER RULE" in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_subpel_temporal_filter_device(None, d, d, d, d, d, 4, 64, None, d, 8, d, 4, st, None) == inv
    assert L.bbme_subpel_temporal_filter_device(None, 0, 0, 64, d, 8, None) == inv
    assert L.bbme_subpel_temporal_filter_chain_device(None, 0, 1, 64, d, 8, 0, None) == inv
    assert L.bbme_get_subpel_temporal_filtered_host(None, 0, 0, 64, d) == inv
    assert L.bbme_subpel_temporal_filter_stats(None, 64, None, st) == inv
    assert hasattr(bbme, "temporal_filter_cells_subpel") and "temporal_filter_cells_subpel" in bbme.__all__
    for name in ("temporal_filter_subpel", "temporal_filter_subpel_stats", "cells_temporal_filter_subpel_device"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        assert hasattr(cls, "get_frame_filtered_subpel")
    assert hasattr(bbme.MFChain, "temporal_filter_run_subpel")
    import inspect
    from blockbasedmotionestimation_amd import sequence
    assert inspect.signature(sequence.denoise_frames).parameters["subpel"].default is False


def test_context_calls_need_a_device(bbme):
    """Without a GPU no context exists to filter on: there is no CPU fallback behind the context-level calls (the rule on the CPU
    is bbme_subpel_temporal_filter_host, asked for by name)."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from blockbasedmotionestimation_amd import _capi
    z = np.zeros((64, 64), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MF(z, z, [32], [16]).temporal_filter_subpel(64)
    assert e.value.status == _capi.ERR_HIP and "no CPU fallback" in e.value.message


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    H, W = 12, 16
    img = np.zeros((H, W), np.uint8)
    g = np.zeros((H // 2, W // 2, 2), np.int16)
    out = np.zeros((H, W), np.uint8)
    wmap = np.zeros((H // 2, W // 2), np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    I, G = img.ctypes.data, g.ctypes.data

    def call(p=I, c=I, n=I, w=W, h=H, gp=G, gn=G, thr=64, win=None, o=out.ctypes.data, m=wmap.ctypes.data, t=st):
        return L.bbme_subpel_temporal_filter_host(p, c, n, w, h, gp, gn, thr, win, o, m, t)

    assert call() == 0
    assert call(p=None, gp=None) == 0 and call(n=None, gn=None) == 0              # each neighbour is optional
    assert call(p=None, gp=None, n=None, gn=None) == inv                          # not both
    assert call(p=None) == inv and call(gp=None) == inv and call(n=None) == inv and call(gn=None) == inv      # plane without grid, ...
    assert call(c=None) == inv
    assert call(o=None, m=None, t=None) == inv                                    # nothing asked for
    assert call(o=None) == 0 and call(m=None) == 0 and call(t=None) == 0 and call(o=None, m=None) == 0 and call(o=None, t=None) == 0
    for thr in (0, -1, 1022, 4096):
        assert call(thr=thr) == inv, thr
    assert call(thr=1) == 0 and call(thr=1021) == 0
    assert call(w=W - 1) == inv and call(h=H - 1) == inv                          # odd sizes
    assert call(w=0) == inv and call(h=0) == inv
    CW, CH = W // 2, H // 2
    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (CW - 1, 0, 2, 2), (0, CH - 1, 2, 2), (0, 0, CW + 1, CH)):
        assert call(win=(C.c_int * 4)(*win)) == inv, win
    assert call(win=(C.c_int * 4)(CW - 2, CH - 2, 2, 2)) == 0
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_subpel(img, img, None, g[:, :4], None)
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_subpel(img, img, None, None, None)            # a plane without its grid
    assert e.value.status == inv


@pytest.mark.parametrize("H0,W0", PLANES)
def test_host_rule_equals_numpy_on_every_fraction(bbme, H0, W0):
    """Grids of up to 14 quarter pels plus far vectors: over the seeds every (fx, fy) class is taken by both neighbours."""
    CH, CW = H0 // 2, W0 // 2
    wins = odd_windows(CH, CW) if CW >= 6 and CH >= 4 else [None]
    wins = [w for w in wins if w is None or (w[0] >= 0 and w[1] >= 0 and w[2] >= 1 and w[3] >= 1)]
    seen = [set(), set()]
    n = 0
    for seed in range(6):
        Cur, P, N = near_frames(H0, W0, 10 * H0 + seed)
        qp, qn = fraction_grids(H0, W0, 100 * W0 + seed)
        for thr in (64, 255, 1021):
            for p, a, q, b in neighbour_sets(P, qp, N, qn):
                exp = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, wins[n % len(wins)], (H0, W0, seed))
                n += 1
                if p is not None and q is not None:
                    fp, fn = fractions_taken(exp[1], qp, qn)
                    seen[0] |= fp
                    seen[1] |= fn
    every = {(a, b) for a in range(4) for b in range(4)}
    assert seen[0] == every and seen[1] == every


@pytest.mark.parametrize("H0,W0", PLANES)
def test_validity_at_every_edge(bbme, H0, W0):
    """A cell on the last valid position takes its neighbour; one a quarter pel (f = 0) or a pixel (f != 0) further out has weight
    0 and keeps C's pixels.  The planes are nearly flat, so that every valid cell passes at strength 1021."""
    rng = np.random.default_rng(H0 + W0)
    Cur, P, N = (rng.integers(100, 104, (H0, W0)).astype(np.uint8) for _ in range(3))
    Q, cells = edge_grid(H0, W0)
    assert sum(v for _, _, v in cells) == 16 and len(cells) == 32
    for p, a, q, b in neighbour_sets(P, Q, N, Q):
        out, wmap, _ = assert_host_equals_numpy(bbme, Cur, p, a, q, b, 1021, None, (H0, W0))
        for cx, cy, valid in cells:
            wp, wn = wmap[cy, cx] & 0x0f, wmap[cy, cx] >> 4
            assert (wp > 0) == (valid and p is not None) and (wn > 0) == (valid and q is not None), (cx, cy, valid)
            if not valid:
                assert np.array_equal(out[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2], Cur[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2])


@pytest.mark.parametrize("H0,W0", [(16, 16), (28, 36)])
def test_int16_extremes_leave_the_frame_alone(bbme, H0, W0):
    rng = np.random.default_rng(7 * H0 + W0)
    Cur, P, N = (rng.integers(0, 256, (H0, W0)).astype(np.uint8) for _ in range(3))
    qp, qn = extreme_grids(H0 // 2, W0 // 2, rng)
    for thr in RULE_THRS:
        for p, a, q, b in neighbour_sets(P, qp, N, qn):
            out, wmap, st = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, None)
            assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)


def assert_property_1(filt, Cur, P, GP, N, GN, thr, window=None):
    """`filt`(Cur, P, 4 GP, N, 4 GN, thr, window) -> (out, map, stats) equals the integer rule on GP and GN"""
    exp = np_temporal_filter(Cur, P, GP, N, GN, thr, window)
    q = [None if g is None else (4 * g.astype(np.int32)).astype(np.int16) for g in (GP, GN)]
    got = filt(Cur, P, q[0], N, q[1], thr, window)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and tuple(got[2]) == exp[2], thr
    return got


@pytest.mark.parametrize("thr", THRS)
def test_property_1_division_by_the_strength(bbme, thr):
    """4 x integer grids on K9's strength table: every cost 0..1020, equal to bbme.temporal_filter_cells bit for bit"""
    Cur, N, cost = thr_table_planes()
    z = np.zeros(cost.shape + (2,), np.int16)
    filt = functools.partial(host, bbme)
    _, wmap, _ = assert_property_1(filt, Cur, None, None, N, z, thr)
    assert np.array_equal(wmap >> 4, thr_table_expected(cost, thr))
    old = bbme.temporal_filter_cells(Cur, None, N, None, z, thr)
    new = bbme.temporal_filter_cells_subpel(Cur, None, N, None, z, thr)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]) and old[2] == new[2]


def test_property_1_division_by_the_weight_sum(bbme):
    """4 x integer grids on K9's weight-sum tables: every S = 9..23 with every residue class"""
    filt = functools.partial(host, bbme)
    Cur, P, N, expect_w = s_table_planes()
    z = np.zeros(expect_w.shape[:2] + (2,), np.int16)
    out, wmap, _ = assert_property_1(filt, Cur, P, z, N, z, 64)
    s_table_check(Cur, P, N, expect_w, out, wmap)
    Cur, P, N, expect_w = s23_table_planes()
    out, wmap, _ = assert_property_1(filt, Cur, P, z, N, z, S23_THR)
    s_table_check(Cur, P, N, expect_w, out, wmap, pairs=[(8, 7)], ends=False)


@pytest.mark.parametrize("H0,W0", [(48, 64), (50, 66), (38, 134)])
def test_property_1_on_random_grids(bbme, H0, W0):
    rng = np.random.default_rng(1000 * H0 + W0)
    Cur = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    P = np.clip(Cur.astype(np.int16) + rng.integers(-3, 4, (H0, W0)) * (rng.random((H0, W0)) < 0.5), 0, 255).astype(np.uint8)
    N = np.clip(Cur.astype(np.int16) + rng.integers(-12, 13, (H0, W0)) * (rng.random((H0, W0)) < 0.3), 0, 255).astype(np.uint8)
    CH, CW = H0 // 2, W0 // 2
    gp, gn = random_grids(CH, CW, rng, reach=1)
    still = rng.random((CH, CW)) < 0.6
    gp[still] = 0
    gn[still] = 0
    big = rng.random((CH, CW)) < 0.1                        # vectors that leave the plane, still inside int16 when multiplied by 4
    gp[big] = (W0, -3)
    gn[big] = (-2, -H0)
    wins = odd_windows(CH, CW)
    filt = functools.partial(host, bbme)
    taken = 0
    for n, thr in enumerate(RULE_THRS + (8, 24)):
        for k, (p, a, q, b) in enumerate(neighbour_sets(P, gp, N, gn)):
            taken += sum(assert_property_1(filt, Cur, p, a, q, b, thr, wins[(n + k) % len(wins)])[2][:2])
    assert taken > 0


def test_property_2_equal_planes_and_zero_grids_keep_the_frame(bbme):
    rng = np.random.default_rng(31)
    H0, W0 = 40, 56
    Cur = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    z = np.zeros((H0 // 2, W0 // 2, 2), np.int16)
    cells = H0 * W0 // 4
    for thr in THRS:
        out, wmap, st = host(bbme, Cur, Cur, z, Cur, z, thr)
        assert np.array_equal(out, Cur) and (wmap == 0x88).all() and st == (cells, cells, 16 * cells, 0)
        out, wmap, st = host(bbme, Cur, None, None, Cur, z, thr)
        assert np.array_equal(out, Cur) and (wmap == 0x80).all() and st == (0, cells, 8 * cells, 0)
        out, wmap, st = host(bbme, Cur, Cur, z, None, None, thr)
        assert np.array_equal(out, Cur) and (wmap == 0x08).all() and st == (cells, 0, 8 * cells, 0)


@pytest.mark.parametrize("thr", (1, 64, 1021))
def test_division_on_sampled_costs(bbme, thr):
    """Every cost 0..1020 from ROUNDED half-pel samples, as the next neighbour and as the previous one"""
    Cur, X, grid, k = sampled_cost_table()
    out, wmap, _ = assert_host_equals_numpy(bbme, Cur, None, None, X, grid, thr)
    sampled_cost_check(k, thr, out, wmap >> 4)
    out, wmap, _ = assert_host_equals_numpy(bbme, Cur, X, grid, None, None, thr)
    sampled_cost_check(k, thr, out, wmap & 0x0f)


# ---- quality: three noisy frames cut from one texture made at 4x resolution, moving a fixed number of quarter pels a frame ----

SIZES = [(128, 96), (160, 112)]
NOISE = [(3, 64), (6, 128), (10, 256)]                      # (sigma, strength)
INTERIOR = 16
WHOLE = [(4, 0), (8, -8)]
HALF = [(2, 2), (6, -2), (10, 6), (14, -10)]
QUARTER = [(1, 3), (5, -7)]
TILES = [((2, 2), (10, 6), (14, -10), (-6, 2))]


@functools.lru_cache(maxsize=None)
def _texture(w, h, seed):
    base = hires_texture(w, h, seed)
    return base * (190.0 / 255.0) + 32.0                     # 32..222: the noise clips nothing


def noisy_subpel_frames(w, h, seed, tiles, sigma):
    """Frames 0, 1, 2 of content that moves tiles' (mx, my) QUARTER pels per frame (frames_of cuts at 0, 1 / 2 and 1 of a motion per
    pair: twice that), Gaussian noise of sigma from default_rng(seed + 2) on frames 0, 1, 2 in this order -> (clean, noisy,
    quarter-pel grid from frame 1 into frame 2)"""
    mo = _motion_field(w, h, tiles)
    clean = frames_of(_texture(w, h, seed), w, h, 2 * mo)
    noise = np.random.default_rng(seed + 2)
    noisy = [np.clip(np.rint(f + noise.normal(0.0, sigma, size=f.shape)), 0, 255).astype(np.uint8) for f in clean]
    return clean, noisy, mo[::2, ::2].astype(np.int64)


def interior_gain(frame, noisy, clean):
    k = (slice(INTERIOR, -INTERIOR), slice(INTERIOR, -INTERIOR))
    return psnr(frame[k], clean[k]) - psnr(noisy[k], clean[k])


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("size", range(len(SIZES)))
@pytest.mark.parametrize("case", WHOLE + HALF + QUARTER + TILES)
def test_quality_against_the_clean_middle_frame(bbme, capsys, case, size, noise):
    """The PSNR gain of the filtered middle frame over the noisy one, interior of 16 pixels: the quarter-pel rule on the true
    quarter-pel grids against the integer rule on them rounded to whole pixels (to_next = (q + 2) >> 2, to_prev = -to_next: the
    form in which the integer rule does best).  The floors are the issue's."""
    w, h = SIZES[size]
    sigma, thr = noise
    tiles = (case,) if isinstance(case[0], int) else case
    clean, (f0, f1, f2), q = noisy_subpel_frames(w, h, 100 + size, tiles, sigma)
    q_next, q_prev = q.astype(np.int16), (-q).astype(np.int16)
    i_next = ((q + 2) >> 2).astype(np.int16)
    i_prev = (-i_next).astype(np.int16)
    new2 = assert_host_equals_numpy(bbme, f1, f0, q_prev, f2, q_next, thr, None, case)
    new1 = assert_host_equals_numpy(bbme, f1, None, None, f2, q_next, thr, None, case)
    old2 = bbme.temporal_filter_cells(f1, f0, f2, i_prev, i_next, thr)
    old1 = bbme.temporal_filter_cells(f1, None, f2, None, i_next, thr)
    g = {name: interior_gain(r[0], f1, clean[1]) for name, r in (("new2", new2), ("new1", new1), ("old2", old2), ("old1", old1))}
    with capsys.disabled():
        print("\nsubpel temporal filter %dx%d motion %s sigma %d strength %d: integer rule two-sided %+.2f dB one-sided %+.2f dB | "
              "quarter-pel rule two-sided %+.2f dB one-sided %+.2f dB | weights %s"
              % (w, h, case, sigma, thr, g["old2"], g["old1"], g["new2"], g["new1"], new2[2][:3]))
    if case in WHOLE:
        assert np.array_equal(new2[0], old2[0]) and np.array_equal(new1[0], old1[0])
        return
    if case in HALF or case in TILES:
        assert g["new2"] >= g["old2"] + 1.5, g
    if case in HALF:
        assert g["new2"] >= 4.5, g
        assert g["new1"] >= g["old1"] + 1.2, g
        assert g["new1"] >= 2.5, g
    if case in QUARTER:
        assert g["new2"] >= g["old2"] + 1.0, g


# (tiles, sigma, strength): the statistics of the integer route and of the quarter-pel route, from the first run
PIPELINE_CASES = {
    (((10, 6),), 3, 64): ((2950, 2863, 27710, 26235), (2988, 2916, 34420, 20350)),
    (((10, 6),), 6, 128): ((3053, 3026, 32907, 45660), (3057, 3032, 36229, 38721)),
    (((10, 6),), 10, 256): ((3072, 3072, 36673, 72419), (3072, 3072, 38664, 64385)),
    (((2, 2), (10, 6), (14, -10), (-6, 2)), 3, 64): ((2907, 2896, 27512, 25546), (2956, 2954, 34234, 20617)),
    (((2, 2), (10, 6), (14, -10), (-6, 2)), 6, 128): ((3040, 3027, 33012, 45131), (3046, 3034, 36236, 38724)),
    (((2, 2), (10, 6), (14, -10), (-6, 2)), 10, 256): ((3069, 3068, 36618, 73560), (3069, 3071, 38583, 64705)),
}


@pytest.mark.parametrize("case", list(PIPELINE_CASES))
def test_pipeline_on_the_oracles_fields(bbme, oracle, capsys, case):
    """The whole route on the CPU, the noise entering estimate and refinement: the oracle's fields (f1, f0) and (f1, f2) on the
    noisy frames, refined by bbme.subpel_cells, then the new rule; against bbme.temporal_filter_cells on the same oracle fields.
    The new route may not be worse than the integer route by more than 0.5 dB.  Measured (integer route / quarter-pel route, gain
    over the noisy frame in dB, sigma 3, 6, 10): motion (10, 6) +0.22 / +5.26, +2.35 / +5.87, +3.70 / +6.10; the half-pel tiles
    +0.58 / +4.67, +2.53 / +5.39, +3.29 / +5.65: the route loses nowhere."""
    tiles, sigma, thr = case
    w, h, search, block = 128, 96, [48, 48], [16, 16]
    clean, (f0, f1, f2), _ = noisy_subpel_frames(w, h, 100, tiles, sigma)
    _, to_prev = _oracle_fields(bbme, oracle, f1, f0, search, block)
    _, to_next = _oracle_fields(bbme, oracle, f1, f2, search, block)
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    P, Cur, N = (bbme.pad_zero(f, px, py) for f in (f0, f1, f2))
    q_prev, _ = bbme.subpel_cells(Cur, P, to_prev)
    q_next, _ = bbme.subpel_cells(Cur, N, to_next)
    old, _, st_old = bbme.temporal_filter_cells(Cur, P, N, to_prev, to_next, thr)
    new, _, st_new = assert_host_equals_numpy(bbme, Cur, P, q_prev, N, q_next, thr, None, "pipeline")
    st_old = tuple(st_old[k] for k in STAT_KEYS)
    crop = (slice(py, py + h), slice(px, px + w))
    g_old, g_new = interior_gain(old[crop], f1, clean[1]), interior_gain(new[crop], f1, clean[1])
    with capsys.disabled():
        print("\nsubpel temporal filter pipeline %dx%d motion %s sigma %d strength %d: integer route %+.2f dB %s | quarter-pel route "
              "%+.2f dB %s" % (w, h, tiles, sigma, thr, g_old, st_old, g_new, st_new))
    assert g_new >= g_old - 0.5, (g_old, g_new)
    assert (st_old, st_new) == PIPELINE_CASES[case]
