"""CPU tests of the temporal filter rule (include/bbme.h, "TEMPORAL FILTER RULE"): the C-ABI exports the temporal filter calls;
bbme_temporal_filter_host follows the rule, which is restated here in vectorised numpy from the header's text and imported by the
GPU tests; closed forms (equal planes, constant planes, a neighbour pointing outside) and every quotient of the two divisions
carry their answers written out; on noisy videos of constant motion the filtered middle frame gains what averaging three aligned
frames should gain."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_bidirectional import CASES, _oracle_fields
from test_interpolation_cpu import (_box5, extreme_grids, odd_windows, oracle_grids, padded_planes, psnr, random_grids)

NEW_SYMBOLS = ["bbme_temporal_filter_host", "bbme_cells_temporal_filter_device", "bbme_temporal_filter_device",
               "bbme_temporal_filter_chain_device", "bbme_get_temporal_filtered_host", "bbme_temporal_filter_stats",
               "bbme_frame_plane_device"]

STAT_KEYS = ("prev_cells", "next_cells", "weight", "change")

THRS = (1, 2, 3, 7, 64, 255, 1020, 1021)                   # the strengths of the division tests
RULE_THRS = (1, 64, 255, 1021)


def np_temporal_filter(Cur, P, GP, N, GN, thr, window=None):
    """The rule of include/bbme.h: output cell (cx, cy) with origin o = (2 cx, 2 cy) looks, for each present neighbour X (P with
    GP, N with GN; a neighbour is present when neither is None), at the 2x2 cell of X at p = o + G[cy, cx]; valid when it lies
    inside the plane; cost = sum |C[o + (j, i)] - X[p + (j, i)]|; w = 8 (thr - cost) // thr when valid and cost < thr, else 0;
    S = 8 + wP + wN and out = (8 C + wP P[pP ..] + wN N[pN ..] + S // 2) // S.  Returns (out uint8 (H0, W0), map uint8 (CH, CW)
    holding wP | wN << 4, (cells with wP > 0, cells with wN > 0, sum of wP + wN, sum of |out - C| over the window's pixels) over
    window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    Cur = np.asarray(Cur).astype(np.int64)
    H0, W0 = Cur.shape
    CH, CW = H0 // 2, W0 // 2
    assert (P is None) == (GP is None) and (N is None) == (GN is None) and (P is not None or N is not None)
    cy, cx = np.mgrid[0:CH, 0:CW]
    ox, oy = 2 * cx, 2 * cy
    cell = np.stack([np.stack([Cur[oy + i, ox + j] for j in range(2)]) for i in range(2)])      # [i, j, cy, cx]
    ws, moved = [], []
    for X, G in ((P, GP), (N, GN)):
        if X is None:
            ws.append(np.zeros((CH, CW), np.int64))
            moved.append(np.zeros((2, 2, CH, CW), np.int64))
            continue
        X = np.asarray(X).astype(np.int64)
        G = np.asarray(G).astype(np.int64)
        px, py = ox + G[..., 0], oy + G[..., 1]
        valid = (px >= 0) & (px <= W0 - 2) & (py >= 0) & (py <= H0 - 2)
        qx, qy = np.where(valid, px, 0), np.where(valid, py, 0)
        m = np.stack([np.stack([X[qy + i, qx + j] for j in range(2)]) for i in range(2)])
        cost = np.abs(cell - m).sum(axis=(0, 1))
        w = np.where(valid & (cost < thr), 8 * (thr - cost) // thr, 0)
        ws.append(w)
        moved.append(m)
    wP, wN = ws
    S = 8 + wP + wN
    pix = (8 * cell + wP * moved[0] + wN * moved[1] + S // 2) // S
    out = np.empty((H0, W0), np.uint8)
    for i in range(2):
        for j in range(2):
            out[i::2, j::2] = pix[i, j]
    change = np.abs(pix - cell).sum(axis=(0, 1))
    if window is None:
        window = (0, 0, CW, CH)
    x0, y0, w, h = window
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    stats = (int((wP[sl] > 0).sum()), int((wN[sl] > 0).sum()), int((wP[sl] + wN[sl]).sum()), int(change[sl].sum()))
    return out, (wP | wN << 4).astype(np.uint8), stats


def host_temporal_filter(bbme, Cur, P, GP, N, GN, thr, window=None):
    out, wmap, st = bbme.temporal_filter_cells(Cur, P, N, GP, GN, thr, window)
    return out, wmap, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, Cur, P, GP, N, GN, thr, window, what=None):
    exp = np_temporal_filter(Cur, P, GP, N, GN, thr, window)
    got = host_temporal_filter(bbme, Cur, P, GP, N, GN, thr, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert np.array_equal(got[0], exp[0]), tag
    assert np.array_equal(got[1], exp[1]), tag
    assert got[2] == exp[2], tag
    return exp


def neighbour_sets(P, GP, N, GN):
    """Both neighbours, then each one alone."""
    return [(P, GP, N, GN), (P, GP, None, None), (None, None, N, GN)]


# ---- the two division tables: planes and grids (zero) on which every numerator of a division occurs ------------------------

def thr_table_planes():
    """C = 0 everywhere and a 46 x 46-cell neighbour plane (92 x 92 pixels) whose cell k <= 1020, in raster order, sums to cost k
    (the rest to 1020): with zero grids the weight is 8 (thr - k) / thr, or 0 from k >= thr."""
    CW = CH = 46
    cost = np.minimum(np.arange(CW * CH), 1020)
    N = np.zeros((2 * CH, 2 * CW), np.uint8)
    px = np.zeros((CW * CH, 4), np.int64)
    rest = cost.copy()
    for q in range(4):
        px[:, q] = np.minimum(rest, 255)
        rest -= px[:, q]
    assert (rest == 0).all()
    px = px.reshape(CH, CW, 4)
    N[0::2, 0::2], N[0::2, 1::2], N[1::2, 0::2], N[1::2, 1::2] = px[..., 0], px[..., 1], px[..., 2], px[..., 3]
    return np.zeros_like(N), N, cost.reshape(CH, CW)


def thr_table_expected(cost, thr):
    return np.where(cost < thr, 8 * (thr - cost) // thr, 0)


# (wP, wN) for every S = 8 .. 24.  At thr = 64, w = 8 (64 - cost) / 64 = (64 - cost) >> 3: a weight w > 0 comes from a cost of
# 8 (8 - w) - 7 .. 8 (8 - w), a weight 0 from 64 or more.  Since 8 = S - wP - wN, a pixel's numerator is
# wP (p - c) + wN (n - c) + S / 2 (mod S) with |p - c| and |n - c| at most the neighbour's cost: it can meet the residues
# s_table_residues() lists and no others.  One weight of each pair is odd wherever a sum allows it, and then that is EVERY class
# mod S for S = 9 .. 22.  Two sums are limited by the rule itself, at every strength: S = 8 (no neighbour: 8 c + 4) meets only 4 and
# S = 24 (both weights 8, which only cost 0 gives: 24 c + 12) only 12.  S = 23 (weights 8 and 7: 7 d + 11) is limited at thr = 64
# only, where a weight 7 means a cost of 1 .. 8 and |d| <= 8 reaches 17 classes: at thr = 1021 a weight 7 means a cost of 1 .. 127,
# and s23_table_planes() meets all 23 there.
S_PAIRS = [(0, 0)] + [(1, s - 1) if s <= 9 else (s - 7, 7) for s in range(1, 16)] + [(8, 8)]


def s_table_residues(wp, wn):
    """The residue classes mod S = 8 + wp + wn that a numerator of a cell with these weights can fall into at thr = 64."""
    S = 8 + wp + wn
    reach = [8 * (8 - w) if w else 0 for w in (wp, wn)]
    return {(wp * d1 + wn * d2 + S // 2) % S for d1 in range(-reach[0], reach[0] + 1) for d2 in range(-reach[1], reach[1] + 1)}


def s_table_planes():
    """A 132 x 100 plane (66 x 50 cells, zero grids, thr = 64): for every S = 8 + wP + wN a band of 2 cell rows.  Cell k of a band
    aims its first pixel at the residue class k mod S: it takes the smallest differences (d1, d2) = (p - c, n - c) with
    wP d1 + wN d2 + S / 2 = k (mod S) that the weights' cost buckets allow (a weight w > 0 needs a cost of 8 (8 - w) - 7 .. 8 (8 - w),
    a weight 0 one of 64 or more); the rest of each neighbour's cost goes to a pixel of its own, the fourth pixel is equal in all
    three planes, and C varies from cell to cell.  Then a row of all-0 cells and rows of all-255 cells, cost 0 and S = 24, for the
    two ends 12 and 255 * 24 + 12.  Returns (C, P, N, the (wP, wN) of every cell)."""
    CW, CH, rows = 66, 50, 2
    Cur = np.zeros((2 * CH, 2 * CW), np.uint8)
    P = np.zeros_like(Cur)
    N = np.zeros_like(Cur)
    expect_w = np.zeros((CH, CW, 2), np.int64)
    for b, (wp, wn) in enumerate(S_PAIRS):
        S = 8 + wp + wn
        lo = [max(0, 8 * (8 - w) - 7) if w else 64 for w in (wp, wn)]    # the smallest cost that gives the weight
        reach = [8 * (8 - w) if w else 0 for w in (wp, wn)]               # the largest, and so the largest |d| (a weight 0 uses nothing)
        pairs = sorted(((d1, d2) for d1 in range(-reach[0], reach[0] + 1) for d2 in range(-reach[1], reach[1] + 1)),
                       key=lambda d: (abs(d[0]) + abs(d[1]), d))
        for k in range(rows * CW):
            cy, cx = b * rows + k // CW, k % CW
            d1, d2 = next((d for d in pairs if (wp * d[0] + wn * d[1] + S // 2 - k) % S == 0), (0, 0))
            c = np.array([64 + (k * 5) % 128, (k * 7 + 3) % 128, (k * 13 + 5) % 128, (2 * k + b) % 256], np.int64)
            cost = [max(lo[0], abs(d1)), max(lo[1], abs(d2))]
            p = c + np.array([d1, cost[0] - abs(d1), 0, 0])
            n = c + np.array([d2, 0, cost[1] - abs(d2), 0])
            for q, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                Cur[2 * cy + i, 2 * cx + j], P[2 * cy + i, 2 * cx + j], N[2 * cy + i, 2 * cx + j] = c[q], p[q], n[q]
            expect_w[cy, cx] = (wp, wn)
    ends = rows * len(S_PAIRS)                              # row `ends` stays all 0, the rows below are all 255
    Cur[2 * ends + 2:], P[2 * ends + 2:], N[2 * ends + 2:] = 255, 255, 255
    expect_w[ends:] = (8, 8)
    return Cur, P, N, expect_w


S23_THR = 1021


def s23_table_planes():
    """A 132 x 100 plane of cells with wP = 8 and wN = 7 at thr = 1021 (zero grids): P = C (cost 0); cell k aims its first pixel at
    the residue class k mod 23 with the smallest d = n - c such that 7 d + 11 = k (mod 23), |d| <= 11, and brings N's cost to at
    least 1 on a pixel of its own (a weight 7 needs a cost of 1 .. 127 here).  Returns (C, P, N, the (wP, wN) of every cell)."""
    CW, CH = 66, 50
    Cur = np.zeros((2 * CH, 2 * CW), np.uint8)
    N = np.zeros_like(Cur)
    for k in range(CW * CH):
        cy, cx = k // CW, k % CW
        d = next(d for d in sorted(range(-11, 12), key=lambda d: (abs(d), d)) if (7 * d + 11 - k) % 23 == 0)
        c = np.array([64 + (k * 5) % 128, (k * 7 + 3) % 128, (k * 13 + 5) % 128, (2 * k) % 256], np.int64)
        n = c + np.array([d, 0, 1 + k % 100 if d == 0 or k % 2 else 0, 0])
        for q, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            Cur[2 * cy + i, 2 * cx + j], N[2 * cy + i, 2 * cx + j] = c[q], n[q]
    expect_w = np.empty((CH, CW, 2), np.int64)
    expect_w[...] = (8, 7)
    return Cur, Cur.copy(), N, expect_w


def s_table_check(Cur, P, N, expect_w, out, wmap, pairs=None, ends=True):
    """The weights are the constructed ones, every S of `pairs` (default: S_PAIRS at thr = 64) occurs with every residue class mod S
    -- but for 8 and 24, which the rule limits, and for 23 at thr = 64, which s23_table_planes() completes -- and out is the exact
    quotient."""
    wp, wn = expect_w[..., 0], expect_w[..., 1]
    assert np.array_equal(wmap, (wp | wn << 4).astype(np.uint8))
    S = 8 + wp + wn
    seen = {}
    for i in range(2):
        for j in range(2):
            num = 8 * Cur[i::2, j::2].astype(np.int64) + wp * P[i::2, j::2] + wn * N[i::2, j::2] + S // 2
            assert np.array_equal(out[i::2, j::2], num // S), (i, j)                # Python-exact in int64
            for s in range(8, 25):
                seen.setdefault(s, set()).update((num[S == s] % s).tolist())
    for wp_, wn_ in S_PAIRS if pairs is None else pairs:
        s = 8 + wp_ + wn_
        if pairs is None and s in (8, 23, 24):
            assert seen[s] == s_table_residues(wp_, wn_), s  # every class the rule can meet at thr = 64 is met
        else:
            assert seen[s] == set(range(s)), s
    if ends:
        rows = 2 * 2 * len(S_PAIRS)
        assert (out[rows:rows + 2] == 0).all() and (out[rows + 2:] == 255).all()


def noisy_motion_video(w, h, seed, mm, tiles, sigma):
    """Three frames of test_interpolation_cpu.constant_motion_video's texture, rescaled to 32..222 so that noise clips nothing:
    frame k shows the tiles x tiles tiles moved by k mv (mv as there, default_rng(seed + 1)); Gaussian noise of `sigma` from
    default_rng(seed + 2).normal on frames 0, 1, 2 in this order.  Returns (clean frames, noisy frames)."""
    m = 2 * mm
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(h + 2 * m, w + 2 * m)).astype(np.float64)
    for _ in range(3):
        base = _box5(base)
    base -= base.min()
    base *= 190 / base.max()
    base = np.rint(base + 32).astype(np.uint8)
    mv = np.random.default_rng(seed + 1).integers(-mm // 2, mm // 2 + 1, size=(tiles, tiles, 2))
    ty = np.minimum(np.arange(h) * tiles // h, tiles - 1)
    tx = np.minimum(np.arange(w) * tiles // w, tiles - 1)
    mo = mv[ty[:, None], tx[None, :]]
    ys, xs = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed + 2)
    clean, noisy = [], []
    for k in (0, 1, 2):
        f = base[ys - k * mo[..., 1] + m, xs - k * mo[..., 0] + m]
        clean.append(f)
        noisy.append(np.clip(np.rint(f + noise.normal(0.0, sigma, size=f.shape)), 0, 255).astype(np.uint8))
    return clean, noisy


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
    assert "TEMPORAL FILTER RULE" in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    p = C.c_void_p()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_temporal_filter_device(None, d, d, d, d, d, 64, None, d, 8, d, 4, st, None) == inv
    assert L.bbme_temporal_filter_device(None, 0, 0, 64, d, 8, None) == inv
    assert L.bbme_temporal_filter_chain_device(None, 0, 1, 64, d, 8, 0, None) == inv
    assert L.bbme_get_temporal_filtered_host(None, 0, 0, 64, d) == inv
    assert L.bbme_temporal_filter_stats(None, 64, None, st) == inv
    assert L.bbme_frame_plane_device(None, 0, 0, 0, C.byref(p)) == inv
    assert hasattr(bbme, "temporal_filter_cells")
    for name in ("temporal_filter", "temporal_filter_stats", "cells_temporal_filter_device", "frame_plane_tensor", "cells_tensor",
                 "backward_cells_tensor"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        assert hasattr(cls, "get_frame_filtered")
    assert hasattr(bbme.MFChain, "temporal_filter_run")
    from blockbasedmotionestimation_amd import sequence
    assert hasattr(sequence, "denoise_frames")


def test_context_calls_need_a_device(bbme):
    """Without a GPU no context exists to filter on: its creation is BBME_ERR_HIP, there is no CPU fallback behind the
    context-level calls (the rule on the CPU is bbme_temporal_filter_host, asked for by name)."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from blockbasedmotionestimation_amd import _capi
    z = np.zeros((64, 64), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MF(z, z, [32], [16]).temporal_filter(64)
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
        return L.bbme_temporal_filter_host(p, c, n, w, h, gp, gn, thr, win, o, m, t)

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
        bbme.temporal_filter_cells(img, img, None, g[:, :4], None)
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells(img, img, None, None, None)                   # a plane without its grid
    assert e.value.status == inv


@pytest.mark.parametrize("name", list(CASES))
def test_host_rule_equals_numpy_on_the_oracles_fields(bbme, oracle, name):
    """Image 1 with image 2 along the forward cells (to_next), image 2 with image 1 along the backward cells (to_prev), and image
    2 between two copies of image 1 (both grids the backward cells): the one frame of a pair that has a grid to use both ways."""
    I1, I2 = padded_planes(bbme, name)
    fwd, bwd = oracle_grids(bbme, oracle, name)
    CH, CW = fwd.shape[:2]
    wins = odd_windows(CH, CW)
    taken = [0, 0]
    for n, thr in enumerate(RULE_THRS):
        win = wins[n % len(wins)]
        e1 = assert_host_equals_numpy(bbme, I1, None, None, I2, fwd, thr, win, name)
        e2 = assert_host_equals_numpy(bbme, I2, I1, bwd, None, None, thr, win, name)
        assert_host_equals_numpy(bbme, I2, I1, bwd, I1, bwd, thr, wins[(n + 1) % len(wins)], name)
        assert not (e1[1] & 0x0f).any() and not (e2[1] & 0xf0).any()              # an absent neighbour has weight 0
        taken[0] += e1[2][1]
        taken[1] += e2[2][0]
    assert taken[0] > 0 and taken[1] > 0


@pytest.mark.parametrize("H0,W0", [(48, 64), (100, 132), (98, 140), (50, 66), (80, 12), (38, 134)])      # CW 32, 66, 70, 33, 6, 67
def test_host_rule_equals_numpy_on_random_grids(bbme, H0, W0):
    rng = np.random.default_rng(1000 * H0 + W0)
    Cur = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    # neighbours near enough for every weight 0..8 to occur at the strengths used
    P = np.clip(Cur.astype(np.int16) + rng.integers(-3, 4, (H0, W0)) * (rng.random((H0, W0)) < 0.5), 0, 255).astype(np.uint8)
    N = np.clip(Cur.astype(np.int16) + rng.integers(-12, 13, (H0, W0)) * (rng.random((H0, W0)) < 0.3), 0, 255).astype(np.uint8)
    CH, CW = H0 // 2, W0 // 2
    gp, gn = random_grids(CH, CW, rng, reach=1)
    still = rng.random((CH, CW)) < 0.6                     # most cells look straight across, where the neighbours are near
    gp[still] = 0
    gn[still] = 0
    wins = odd_windows(CH, CW)
    seen = set()
    for n, thr in enumerate(RULE_THRS + (8, 24)):
        for k, (p, a, q, b) in enumerate(neighbour_sets(P, gp, N, gn)):
            exp = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, wins[(n + k) % len(wins)])
            seen |= set(np.unique(exp[1] & 0x0f).tolist()) | set(np.unique(exp[1] >> 4).tolist())
    assert seen == set(range(9))


@pytest.mark.parametrize("H0,W0", [(48, 64), (34, 60)])
def test_int16_extremes_leave_the_frame_alone(bbme, H0, W0):
    rng = np.random.default_rng(7 * H0 + W0)
    Cur, P, N = (rng.integers(0, 256, (H0, W0)).astype(np.uint8) for _ in range(3))
    gp, gn = extreme_grids(H0 // 2, W0 // 2, rng)
    for thr in RULE_THRS:
        for p, a, q, b in neighbour_sets(P, gp, N, gn):
            out, wmap, st = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, None)
            assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)


def test_equal_planes_and_zero_grids_keep_the_frame(bbme):
    rng = np.random.default_rng(31)
    H0, W0 = 40, 56
    Cur = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    z = np.zeros((H0 // 2, W0 // 2, 2), np.int16)
    cells = H0 * W0 // 4
    for thr in THRS:
        out, wmap, st = host_temporal_filter(bbme, Cur, Cur, z, Cur, z, thr)
        assert np.array_equal(out, Cur) and (wmap == 0x88).all() and st == (cells, cells, 16 * cells, 0)
        out, wmap, st = host_temporal_filter(bbme, Cur, None, None, Cur, z, thr)
        assert np.array_equal(out, Cur) and (wmap == 0x80).all() and st == (0, cells, 8 * cells, 0)
        assert np_temporal_filter(Cur, Cur, z, Cur, z, thr)[2] == (cells, cells, 16 * cells, 0)


@pytest.mark.parametrize("a,b,c", [(100, 100, 100), (90, 100, 112), (0, 3, 255), (255, 250, 251), (10, 10, 17), (31, 30, 14)])
def test_constant_planes(bbme, a, b, c):
    """Planes P = a, C = b, N = c with zero grids: every cell costs 4 |b - a| and 4 |b - c|, and the answer is one number."""
    H0, W0 = 24, 36
    P, Cur, N = (np.full((H0, W0), v, np.uint8) for v in (a, b, c))
    z = np.zeros((H0 // 2, W0 // 2, 2), np.int16)
    cells = H0 * W0 // 4
    for thr in THRS:
        cp, cn = 4 * abs(b - a), 4 * abs(b - c)
        wp = 8 * (thr - cp) // thr if cp < thr else 0
        wn = 8 * (thr - cn) // thr if cn < thr else 0
        S = 8 + wp + wn
        v = (8 * b + wp * a + wn * c + S // 2) // S
        out, wmap, st = host_temporal_filter(bbme, Cur, P, z, N, z, thr)
        assert (out == v).all() and (wmap == (wp | wn << 4)).all(), (thr, v, wp, wn)
        assert st == (cells * (wp > 0), cells * (wn > 0), cells * (wp + wn), 4 * cells * abs(v - b))


def test_one_sided_equals_two_sided_with_the_other_grid_outside(bbme):
    rng = np.random.default_rng(77)
    H0, W0 = 44, 60
    Cur = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    P = np.clip(Cur.astype(np.int16) + rng.integers(-4, 5, (H0, W0)), 0, 255).astype(np.uint8)
    N = np.clip(Cur.astype(np.int16) + rng.integers(-4, 5, (H0, W0)), 0, 255).astype(np.uint8)
    CH, CW = H0 // 2, W0 // 2
    gp, gn = random_grids(CH, CW, rng, reach=1)
    away = np.empty((CH, CW, 2), np.int16)
    away[...] = (W0, -H0)                                   # every cell's target lies outside the plane
    for thr in (24, 64, 1021):
        one = host_temporal_filter(bbme, Cur, None, None, N, gn, thr)
        two = host_temporal_filter(bbme, Cur, P, away, N, gn, thr)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2]
        one = host_temporal_filter(bbme, Cur, P, gp, None, None, thr)
        two = host_temporal_filter(bbme, Cur, P, gp, N, away, thr)
        assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2]
        assert one[2][0] > 0


@pytest.mark.parametrize("thr", THRS)
def test_division_by_the_strength_is_exact(bbme, thr):
    Cur, N, cost = thr_table_planes()
    z = np.zeros(cost.shape + (2,), np.int16)
    exp = thr_table_expected(cost, thr)
    _, wmap, _ = host_temporal_filter(bbme, Cur, None, None, N, z, thr)
    assert np.array_equal(wmap >> 4, exp) and not (wmap & 0x0f).any()
    _, wmap, _ = host_temporal_filter(bbme, Cur, N, z, None, None, thr)
    assert np.array_equal(wmap, exp)
    assert (exp == 8).sum() == 1 and exp[0, 0] == 8           # w = 8 only at cost 0


def test_division_by_the_weight_sum_is_exact(bbme):
    Cur, P, N, expect_w = s_table_planes()
    z = np.zeros(expect_w.shape[:2] + (2,), np.int16)
    out, wmap, _ = host_temporal_filter(bbme, Cur, P, z, N, z, 64)
    s_table_check(Cur, P, N, expect_w, out, wmap)
    exp = np_temporal_filter(Cur, P, z, N, z, 64)
    assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1])
    # S = 23 with all of its classes, at the strength that allows them
    Cur, P, N, expect_w = s23_table_planes()
    out, wmap, _ = host_temporal_filter(bbme, Cur, P, z, N, z, S23_THR)
    s_table_check(Cur, P, N, expect_w, out, wmap, pairs=[(8, 7)], ends=False)
    exp = np_temporal_filter(Cur, P, z, N, z, S23_THR)
    assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1])


# (w, h, search, block, seed, mm, tiles)
QUALITY_VIDEOS = [(128, 96, (48, 48), (16, 16), 11, 12, 2), (192, 128, (40, 40), (8, 8), 13, 8, 3), (256, 192, (48, 48), (16, 16), 14, 12, 4)]
QUALITY_NOISE = [(3, 64), (6, 128), (10, 256)]              # (sigma, strength)


@pytest.mark.parametrize("noise", QUALITY_NOISE)
@pytest.mark.parametrize("video", QUALITY_VIDEOS)
def test_filtered_middle_frame_gains_on_the_noisy_one(bbme, oracle, video, noise):
    """Noisy frames f0, f1, f2 of constant motion, the oracle's fields (f1, f0) and (f1, f2) estimated on the noisy frames
    themselves: over the interior the PSNR of the filtered f1 against the clean f1 beats the noisy f1's by at least 3.0 dB with
    both neighbours and 1.5 dB with the next one alone (three equal weights would reach 10 log10 3 = 4.77 dB, two 3.01 dB; a
    swapped neighbour or sign loses whole decibels against the noisy frame).
    Measured with this file's restatement (two-sided / one-sided gain in dB), videos in the order of QUALITY_VIDEOS:
        sigma 3, strength 64:    3.94 / 2.13,  3.88 / 2.30,  4.00 / 2.08
        sigma 6, strength 128:   3.93 / 2.12,  3.98 / 2.36,  4.11 / 2.24
        sigma 10, strength 256:  3.82 / 1.99,  3.82 / 2.27,  4.09 / 2.27
    """
    w, h, search, block, seed, mm, tiles = video
    sigma, thr = noise
    search, block = list(search), list(block)
    clean, (f0, f1, f2) = noisy_motion_video(w, h, seed, mm, tiles, sigma)
    _, to_prev = _oracle_fields(bbme, oracle, f1, f0, search, block)
    _, to_next = _oracle_fields(bbme, oracle, f1, f2, search, block)
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    P, Cur, N = (bbme.pad_zero(f, px, py) for f in (f0, f1, f2))
    two = assert_host_equals_numpy(bbme, Cur, P, to_prev, N, to_next, thr, None)
    one = assert_host_equals_numpy(bbme, Cur, None, None, N, to_next, thr, None)
    inner = (slice(mm, h - mm), slice(mm, w - mm))
    crop = (slice(py, py + h), slice(px, px + w))
    p_noisy = psnr(f1[inner], clean[1][inner])
    p_two, p_one = psnr(two[0][crop][inner], clean[1][inner]), psnr(one[0][crop][inner], clean[1][inner])
    print("video %s sigma %d strength %d: noisy %.2f dB, two-sided +%.2f dB, one-sided +%.2f dB, weights %s"
          % (video, sigma, thr, p_noisy, p_two - p_noisy, p_one - p_noisy, two[2][:3]))
    assert p_two >= p_noisy + 3.0, (p_two, p_noisy)
    assert p_one >= p_noisy + 1.5, (p_one, p_noisy)
