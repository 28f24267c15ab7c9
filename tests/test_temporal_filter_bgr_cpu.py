"""CPU tests of the BGR temporal filter rule (include/bbme.h, "BGR TEMPORAL FILTER RULE"): the C-ABI exports the colour calls;
bbme_temporal_filter_bgr_host follows the rule, which is restated here in vectorised numpy from the header's text and imported by
the GPU tests; on B = G = R it is the grey rule; the cost is the largest per-channel SAD, not the luma's; every quotient of the two
divisions occurs in every channel; on noisy colour videos the filtered middle frame gains in every channel what the grey filter
gains in grey, and weights taken from the luma do worse."""
import ctypes as C
import os

import numpy as np
import pytest

from test_bgr_cpu import SHAPES, colour_pair, np_bgr_to_gray
from test_gpu_bidirectional import _oracle_fields
from test_interpolation_cpu import _box5, extreme_grids, odd_windows, psnr, random_grids
from test_temporal_filter_cpu import (QUALITY_NOISE, QUALITY_VIDEOS, S23_THR, STAT_KEYS, THRS, neighbour_sets, np_temporal_filter,
                                      s23_table_planes, s_table_check, s_table_planes, thr_table_expected, thr_table_planes)

NEW_SYMBOLS = ["bbme_temporal_filter_bgr_host", "bbme_cells_temporal_filter_bgr_device", "bbme_temporal_filter_bgr_device",
               "bbme_temporal_filter_bgr_chain_device", "bbme_get_temporal_filtered_bgr_host", "bbme_temporal_filter_bgr_stats"]

RULE_THRS = (1, 64, 255, 1021)


def np_temporal_filter_bgr(Cur, P, GP, N, GN, thr, pad_x, pad_y, window=None):
    """The rule of include/bbme.h: every (H, W, 3) frame is read as if zero-padded by (pad_x, pad_y) to H0 x W0; cell (cx, cy)
    with origin o = (2 cx, 2 cy) looks, for each present neighbour X (P with GP, N with GN), at the 2x2 cell of X at
    p = o + G[cy, cx], valid when it lies inside the padded view; cost_c = sum |C[o + (j, i)][c] - X[p + (j, i)][c]| per channel,
    cost = max over the channels; w = 8 (thr - cost) // thr when valid and cost < thr, else 0; S = 8 + wP + wN and every channel
    of out = (8 C + wP P[pP ..] + wN N[pN ..] + S // 2) // S.  Returns (the unpadded (H, W, 3) uint8 frame, map uint8 (CH, CW)
    holding wP | wN << 4, (cells with wP > 0, cells with wN > 0, sum of wP + wN, sum of |out - C| over the window's cells' pixels
    and channels on the padded view) over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    H, W = np.asarray(Cur).shape[:2]

    def padded(F):
        return np.pad(np.asarray(F).astype(np.int64), ((pad_y, pad_y), (pad_x, pad_x), (0, 0)))

    Cur = padded(Cur)
    H0, W0 = Cur.shape[:2]
    assert H0 % 2 == 0 and W0 % 2 == 0
    CH, CW = H0 // 2, W0 // 2
    assert (P is None) == (GP is None) and (N is None) == (GN is None) and (P is not None or N is not None)
    cy, cx = np.mgrid[0:CH, 0:CW]
    ox, oy = 2 * cx, 2 * cy
    cell = np.stack([np.stack([Cur[oy + i, ox + j] for j in range(2)]) for i in range(2)])      # [i, j, cy, cx, channel]
    ws, moved = [], []
    for X, G in ((P, GP), (N, GN)):
        if X is None:
            ws.append(np.zeros((CH, CW), np.int64))
            moved.append(np.zeros((2, 2, CH, CW, 3), np.int64))
            continue
        X = padded(X)
        G = np.asarray(G).astype(np.int64)
        px, py = ox + G[..., 0], oy + G[..., 1]
        valid = (px >= 0) & (px <= W0 - 2) & (py >= 0) & (py <= H0 - 2)
        qx, qy = np.where(valid, px, 0), np.where(valid, py, 0)
        m = np.stack([np.stack([X[qy + i, qx + j] for j in range(2)]) for i in range(2)])
        cost = np.abs(cell - m).sum(axis=(0, 1)).max(axis=-1)
        ws.append(np.where(valid & (cost < thr), 8 * (thr - cost) // thr, 0))
        moved.append(m)
    wP, wN = ws
    S = (8 + wP + wN)[..., None]
    pix = (8 * cell + wP[..., None] * moved[0] + wN[..., None] * moved[1] + S // 2) // S
    full = np.empty((H0, W0, 3), np.uint8)
    for i in range(2):
        for j in range(2):
            full[i::2, j::2] = pix[i, j]
    change = np.abs(pix - cell).sum(axis=(0, 1, 4))
    if window is None:
        window = (0, 0, CW, CH)
    x0, y0, w, h = window
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    stats = (int((wP[sl] > 0).sum()), int((wN[sl] > 0).sum()), int((wP[sl] + wN[sl]).sum()), int(change[sl].sum()))
    return np.ascontiguousarray(full[pad_y:pad_y + H, pad_x:pad_x + W]), (wP | wN << 4).astype(np.uint8), stats


def host_temporal_filter_bgr(bbme, Cur, P, GP, N, GN, thr, pad_x, pad_y, window=None):
    out, wmap, st = bbme.temporal_filter_cells_bgr(Cur, P, N, GP, GN, thr, pad_x, pad_y, window)
    return out, wmap, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, Cur, P, GP, N, GN, thr, pad_x, pad_y, window, what=None):
    exp = np_temporal_filter_bgr(Cur, P, GP, N, GN, thr, pad_x, pad_y, window)
    got = host_temporal_filter_bgr(bbme, Cur, P, GP, N, GN, thr, pad_x, pad_y, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert np.array_equal(got[0], exp[0]), tag
    assert np.array_equal(got[1], exp[1]), tag
    assert got[2] == exp[2], tag
    return exp


def near_colour_triple(w, h, seed):
    """A random colour frame (test_bgr_cpu.colour_pair's first, with its flat patch) and two neighbours near it: P within +-3 on
    half of the samples, N within +-12 on a third, so that every weight 0..8 occurs at the strengths used."""
    Cur, _ = colour_pair(w, h, seed)
    rng = np.random.default_rng(seed + 1)
    P = np.clip(Cur.astype(np.int16) + rng.integers(-3, 4, Cur.shape) * (rng.random(Cur.shape) < 0.5), 0, 255).astype(np.uint8)
    N = np.clip(Cur.astype(np.int16) + rng.integers(-12, 13, Cur.shape) * (rng.random(Cur.shape) < 0.3), 0, 255).astype(np.uint8)
    return Cur, P, N


def near_grids(CH, CW, rng):
    """random_grids of reach 1 with most cells looking straight across, where the neighbours are near."""
    gp, gn = random_grids(CH, CW, rng, reach=1)
    still = rng.random((CH, CW)) < 0.6
    gp[still] = 0
    gn[still] = 0
    return gp, gn


def in_channel(plane, k, rest):
    """The (H, W, 3) frame with `plane` in channel k and `rest` in the two others."""
    f = np.empty(plane.shape + (3,), np.uint8)
    f[...] = np.asarray(rest)[..., None]
    f[..., k] = plane
    return f


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
        assert "int %s(" % name in header, name
    assert "BGR TEMPORAL FILTER RULE" in header
    assert "is a follow-up" not in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_temporal_filter_bgr_device(None, d, d, d, 24, d, d, 64, None, d, 24, d, 4, st, None) == inv
    assert L.bbme_temporal_filter_bgr_device(None, 0, 0, 64, d, 24, None) == inv
    assert L.bbme_temporal_filter_bgr_chain_device(None, 0, 1, 64, d, 24, 0, None) == inv
    assert L.bbme_get_temporal_filtered_bgr_host(None, 0, 0, 64, d) == inv
    assert L.bbme_temporal_filter_bgr_stats(None, 64, None, st) == inv
    assert hasattr(bbme, "temporal_filter_cells_bgr") and "temporal_filter_cells_bgr" in bbme.__all__
    for name in ("temporal_filter_bgr", "temporal_filter_bgr_stats", "cells_temporal_filter_bgr_device", "frame_bgr_tensor"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        assert hasattr(cls, "get_frame_filtered_bgr")
    assert hasattr(bbme.MFChain, "temporal_filter_run_bgr")


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    H, W, px, py = 10, 14, 1, 1                                # the padded view is 16 x 12
    img = np.zeros((H, W, 3), np.uint8)
    CH, CW = (H + 2 * py) // 2, (W + 2 * px) // 2
    g = np.zeros((CH, CW, 2), np.int16)
    out = np.zeros((H, W, 3), np.uint8)
    wmap = np.zeros((CH, CW), np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    I, G = img.ctypes.data, g.ctypes.data

    def call(p=I, c=I, n=I, w=W, h=H, px=px, py=py, gp=G, gn=G, thr=64, win=None, o=out.ctypes.data, m=wmap.ctypes.data, t=st):
        return L.bbme_temporal_filter_bgr_host(p, c, n, w, h, px, py, gp, gn, thr, win, o, m, t)

    assert call() == 0
    assert call(p=None, gp=None) == 0 and call(n=None, gn=None) == 0              # each neighbour is optional
    assert call(p=None, gp=None, n=None, gn=None) == inv                          # not both
    assert call(p=None) == inv and call(gp=None) == inv and call(n=None) == inv and call(gn=None) == inv      # frame without grid, ...
    assert call(c=None) == inv
    assert call(o=None, m=None, t=None) == inv                                    # nothing asked for
    assert call(o=None) == 0 and call(m=None) == 0 and call(t=None) == 0 and call(o=None, m=None) == 0 and call(o=None, t=None) == 0
    for thr in (0, -1, 1022, 4096):
        assert call(thr=thr) == inv, thr
    assert call(thr=1) == 0 and call(thr=1021) == 0
    assert call(w=W - 1) == inv and call(h=H - 1) == inv                          # an odd W0, an odd H0
    assert call(w=0) == inv and call(h=0) == inv
    assert call(px=-1) == inv and call(py=-1) == inv and call(px=-1, w=W + 4) == inv      # negative pads, W0 even or not
    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (CW - 1, 0, 2, 2), (0, CH - 1, 2, 2), (0, 0, CW + 1, CH)):
        assert call(win=(C.c_int * 4)(*win)) == inv, win
    assert call(win=(C.c_int * 4)(CW - 2, CH - 2, 2, 2)) == 0
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_bgr(img, img, None, g[:, :4], None, 64, px, py)
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_bgr(img, img, None, None, None, 64, px, py)   # a frame without its grid
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_bgr(img, img, None, g, None, 64, 0, py)       # 14 x 12: the grid is of another geometry
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_bgr(img[:, :13], img[:, :13], None, g, None, 64, px, py)      # W0 = 15
    assert e.value.status == inv


@pytest.mark.parametrize("shape", list(SHAPES))
def test_host_rule_equals_numpy(bbme, shape):
    """Random grids (most cells near, some leaving the view on every side), both neighbours and each alone, the four strengths,
    full and odd windows: frame, map and statistics."""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    Cur, P, N = near_colour_triple(w, h, 7 * w + h)
    CH, CW = H0 // 2, W0 // 2
    rng = np.random.default_rng(3 * w + h)
    gp, gn = near_grids(CH, CW, rng)
    wins = odd_windows(CH, CW)
    seen = set()
    for n, thr in enumerate(RULE_THRS + (8, 24)):
        for k, (p, a, q, b) in enumerate(neighbour_sets(P, gp, N, gn)):
            exp = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, px, py, wins[(n + k) % len(wins)], shape)
            seen |= set(np.unique(exp[1] & 0x0f).tolist()) | set(np.unique(exp[1] >> 4).tolist())
    assert seen == set(range(9))
    # far vectors as well: random_grids' own reach
    fp, fn = random_grids(CH, CW, rng)
    for thr in (64, 1021):
        assert_host_equals_numpy(bbme, Cur, P, fp, N, fn, thr, px, py, wins[1], shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_int16_extremes_leave_the_frame_alone(bbme, shape):
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    rng = np.random.default_rng(11 * w + h)
    Cur, P, N = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3))
    gp, gn = extreme_grids(H0 // 2, W0 // 2, rng)
    for thr in RULE_THRS:
        for p, a, q, b in neighbour_sets(P, gp, N, gn):
            out, wmap, st = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, px, py, None)
            assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_gray_frames_give_the_grey_result_in_every_channel(bbme, shape):
    """B = G = R: every channel is the unpadded window of bbme.temporal_filter_cells on the zero-padded plane, the map and the
    first three statistics are the grey ones and the fourth is three times the grey one."""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    rng = np.random.default_rng(5 * w + h)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    gP = np.clip(g.astype(np.int16) + rng.integers(-3, 4, g.shape), 0, 255).astype(np.uint8)
    gN = np.clip(g.astype(np.int16) + rng.integers(-9, 10, g.shape) * (rng.random(g.shape) < 0.4), 0, 255).astype(np.uint8)
    CH, CW = H0 // 2, W0 // 2
    gp, gn = near_grids(CH, CW, rng)
    wins = odd_windows(CH, CW)
    grey3 = lambda a: np.repeat(a[..., None], 3, axis=2)
    taken = 0
    for n, thr in enumerate(RULE_THRS):
        win = wins[n % len(wins)]
        for p, a, q, b in neighbour_sets(gP, gp, gN, gn):
            pad = lambda f: None if f is None else bbme.pad_zero(f, px, py)
            eo, em, es = bbme.temporal_filter_cells(pad(g), pad(p), pad(q), a, b, thr, win)
            es = tuple(es[k] for k in STAT_KEYS)
            out, wmap, st = host_temporal_filter_bgr(bbme, grey3(g), None if p is None else grey3(p), a,
                                                     None if q is None else grey3(q), b, thr, px, py, win)
            for k in range(3):
                assert np.array_equal(out[..., k], eo[py:py + h, px:px + w]), (shape, thr, k)
            assert np.array_equal(wmap, em)
            assert st == (es[0], es[1], es[2], 3 * es[3])
            taken += es[2]
    assert taken > 0


@pytest.mark.parametrize("k", [0, 1, 2])
def test_the_cost_is_the_largest_channels(bbme, k):
    """A neighbour that differs from C by d per pixel in channel k alone: the weight is that of cost 4 d, whichever the channel.
    With d = 20 at thr = 64 the LUMA's SAD (about 4 x 2, 4 x 12 or 4 x 6) is below the strength, the channel's 80 is not: weight 0."""
    H, W = 12, 16
    rng = np.random.default_rng(40 + k)
    Cur = rng.integers(0, 200, (H, W, 3), dtype=np.uint8)
    z = np.zeros((H // 2, W // 2, 2), np.int16)
    for d, thr in ((1, 64), (3, 64), (7, 64), (15, 64), (16, 64), (20, 64), (20, 81), (50, 1021), (0, 1)):
        X = Cur.copy()
        X[..., k] += d
        cost = 4 * d
        w = 8 * (thr - cost) // thr if cost < thr else 0
        for P, GP, N, GN in ((X, z, None, None), (None, None, X, z)):
            out, wmap, st = host_temporal_filter_bgr(bbme, Cur, P, GP, N, GN, thr, 0, 0)
            assert (wmap == (w if P is not None else w << 4)).all(), (k, d, thr, w)
            exp = Cur.astype(np.int64)
            exp[..., k] = (8 * exp[..., k] + w * (exp[..., k] + d) + (8 + w) // 2) // (8 + w)
            assert np.array_equal(out, exp)
    X = Cur.copy()
    X[..., k] += 20
    luma_sad = np.abs(np_bgr_to_gray(X).astype(int) - np_bgr_to_gray(Cur).astype(int)).reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
    assert luma_sad.max() < 64                                  # the luma's weights would have let every cell pass
    _, wmap, _ = host_temporal_filter_bgr(bbme, Cur, None, None, X, z, 64, 0, 0)
    assert not wmap.any()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_divisions_are_exact_in_every_channel(bbme, k):
    """The grey tests' tables (every cost 0..1020 at the eight strengths; every S = 9..23 with every residue class) in channel k,
    the two other channels carrying C's own values in all three frames: channel k is the grey table's output."""
    Cur, N, cost = thr_table_planes()
    z = np.zeros(cost.shape + (2,), np.int16)
    rest = (np.arange(Cur.size).reshape(Cur.shape) * 7 % 251).astype(np.uint8)
    fC, fN = in_channel(Cur, k, rest), in_channel(N, k, rest)
    for thr in THRS:
        exp = thr_table_expected(cost, thr)
        out, wmap, _ = host_temporal_filter_bgr(bbme, fC, None, None, fN, z, thr, 0, 0)
        assert np.array_equal(wmap >> 4, exp) and not (wmap & 0x0f).any(), thr
        grey = np_temporal_filter(Cur, None, None, N, z, thr)[0]
        assert np.array_equal(out[..., k], grey), thr
        for o in range(3):
            if o != k:
                assert np.array_equal(out[..., o], rest)       # equal in all frames: untouched at every weight
    for planes, thr, pairs, ends in ((s_table_planes(), 64, None, True), (s23_table_planes(), S23_THR, [(8, 7)], False)):
        Cur, P, N, expect_w = planes
        z = np.zeros(expect_w.shape[:2] + (2,), np.int16)
        rest = (np.arange(Cur.size).reshape(Cur.shape) * 5 % 256).astype(np.uint8)
        out, wmap, _ = host_temporal_filter_bgr(bbme, in_channel(Cur, k, rest), in_channel(P, k, rest), z, in_channel(N, k, rest), z,
                                                thr, 0, 0)
        s_table_check(Cur, P, N, expect_w, out[..., k], wmap, pairs=pairs, ends=ends)
        exp = np_temporal_filter_bgr(in_channel(Cur, k, rest), in_channel(P, k, rest), z, in_channel(N, k, rest), z, thr, 0, 0)
        assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1])


def noisy_motion_bgr_video(w, h, seed, mm, tiles, sigma):
    """test_temporal_filter_cpu.noisy_motion_video in colour: per channel ch a base texture from default_rng(seed + 100 (ch + 1)),
    box-filtered three times and rescaled to 32..222; tile motion from default_rng(seed + 1); ONE default_rng(seed + 2) drawing
    the Gaussian noise channel by channel (B, G, R), within a channel frame by frame (0, 1, 2).  Returns (clean, noisy) frames."""
    m = 2 * mm
    mv = np.random.default_rng(seed + 1).integers(-mm // 2, mm // 2 + 1, size=(tiles, tiles, 2))
    ty = np.minimum(np.arange(h) * tiles // h, tiles - 1)
    tx = np.minimum(np.arange(w) * tiles // w, tiles - 1)
    mo = mv[ty[:, None], tx[None, :]]
    ys, xs = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed + 2)
    clean = [np.empty((h, w, 3), np.uint8) for _ in range(3)]
    noisy = [np.empty((h, w, 3), np.uint8) for _ in range(3)]
    for ch in range(3):
        base = np.random.default_rng(seed + 100 * (ch + 1)).integers(0, 256, size=(h + 2 * m, w + 2 * m)).astype(np.float64)
        for _ in range(3):
            base = _box5(base)
        base -= base.min()
        base *= 190 / base.max()
        base = np.rint(base + 32).astype(np.uint8)
        for k in (0, 1, 2):
            f = base[ys - k * mo[..., 1] + m, xs - k * mo[..., 0] + m]
            clean[k][..., ch] = f
            noisy[k][..., ch] = np.clip(np.rint(f + noise.normal(0.0, sigma, size=f.shape)), 0, 255)
    return clean, noisy


def luma_weighted(Cur, P, GP, N, GN, thr, pad_x, pad_y):
    """The variant the rule replaces: the weights of the grey rule on the luma planes (np_temporal_filter's map) applied to the
    B,G,R frames cell by cell."""
    lum = [None if f is None else np.pad(np_bgr_to_gray(f), ((pad_y, pad_y), (pad_x, pad_x))) for f in (Cur, P, N)]
    _, wmap, _ = np_temporal_filter(lum[0], lum[1], GP, lum[2], GN, thr)
    H, W = Cur.shape[:2]

    pad = lambda F: np.pad(np.asarray(F).astype(np.int64), ((pad_y, pad_y), (pad_x, pad_x), (0, 0)))
    C0 = pad(Cur)
    H0, W0 = C0.shape[:2]
    cy, cx = np.mgrid[0:H0 // 2, 0:W0 // 2]
    acc = np.zeros((2, 2) + wmap.shape + (3,), np.int64)
    for X, G, w in ((P, GP, wmap & 0x0f), (N, GN, wmap >> 4)):
        if X is None:
            continue
        X = pad(X)
        w = w.astype(np.int64)
        qx = np.where(w > 0, 2 * cx + G[..., 0], 0)          # a weight > 0 means a valid p
        qy = np.where(w > 0, 2 * cy + G[..., 1], 0)
        for i in range(2):
            for j in range(2):
                acc[i, j] += w[..., None] * X[qy + i, qx + j]
    S = (8 + (wmap & 0x0f).astype(np.int64) + (wmap >> 4))[..., None]
    full = np.empty_like(C0)
    for i in range(2):
        for j in range(2):
            full[i::2, j::2] = (8 * C0[i::2, j::2] + acc[i, j] + S // 2) // S
    return full[pad_y:pad_y + H, pad_x:pad_x + W].astype(np.uint8)


@pytest.mark.parametrize("noise", QUALITY_NOISE)
@pytest.mark.parametrize("video", QUALITY_VIDEOS)
def test_filtered_middle_frame_gains_in_every_channel(bbme, oracle, video, noise):
    """Noisy colour frames f0, f1, f2 of constant motion, one independent texture per channel, the oracle's fields (f1, f0) and
    (f1, f2) estimated on the LUMA of the noisy frames: over the interior the PSNR of the filtered f1 against the clean f1 beats
    the noisy f1's by at least 3.0 dB with both neighbours and 1.5 dB with the next one alone -- the grey test's floors -- in EVERY
    channel, and the luma-weighted variant (the grey rule's weights on the luma, applied to B, G and R) does worse than the rule
    in its worst channel, two-sided and one-sided.
    Measured with this file's restatement, worst channel, two-sided / one-sided gain in dB (in brackets: the luma-weighted
    variant's), videos in the order of QUALITY_VIDEOS:
        sigma 3, strength 64:    3.91 / 2.22 (0.71 / -1.33),  3.90 / 2.31 (2.04 / 0.29),  4.01 / 2.14 (0.84 / -1.03)
        sigma 6, strength 128:   3.90 / 2.18 (2.48 / 0.53),   4.01 / 2.39 (3.41 / 1.78),  4.07 / 2.21 (2.62 / 0.74)
        sigma 10, strength 256:  3.94 / 2.15 (3.36 / 1.44),   4.08 / 2.39 (3.91 / 2.25),  4.02 / 2.24 (3.42 / 1.62)
    """
    w, h, search, block, seed, mm, tiles = video
    sigma, thr = noise
    search, block = list(search), list(block)
    clean, (f0, f1, f2) = noisy_motion_bgr_video(w, h, seed, mm, tiles, sigma)
    y0, y1, y2 = (np_bgr_to_gray(f) for f in (f0, f1, f2))
    _, to_prev = _oracle_fields(bbme, oracle, y1, y0, search, block)
    _, to_next = _oracle_fields(bbme, oracle, y1, y2, search, block)
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    two = assert_host_equals_numpy(bbme, f1, f0, to_prev, f2, to_next, thr, px, py, None)[0]
    one = assert_host_equals_numpy(bbme, f1, None, None, f2, to_next, thr, px, py, None)[0]
    two_l = luma_weighted(f1, f0, to_prev, f2, to_next, thr, px, py)
    one_l = luma_weighted(f1, None, None, f2, to_next, thr, px, py)
    inner = (slice(mm, h - mm), slice(mm, w - mm))
    gains = {}
    for name, f in (("two", two), ("one", one), ("two_luma", two_l), ("one_luma", one_l)):
        gains[name] = [psnr(f[inner][..., ch], clean[1][inner][..., ch]) - psnr(f1[inner][..., ch], clean[1][inner][..., ch])
                       for ch in range(3)]
    print("video %s sigma %d strength %d, gain in dB over the noisy frame (B, G, R): two-sided %s, one-sided %s; luma-weighted "
          "two-sided %s, one-sided %s" % ((video, sigma, thr) + tuple(" ".join("%+.2f" % g for g in gains[n])
                                                                      for n in ("two", "one", "two_luma", "one_luma"))))
    for ch in range(3):
        assert gains["two"][ch] >= 3.0, (ch, gains["two"])
        assert gains["one"][ch] >= 1.5, (ch, gains["one"])
    assert min(gains["two_luma"]) < min(gains["two"])
    assert min(gains["one_luma"]) < min(gains["one"])
