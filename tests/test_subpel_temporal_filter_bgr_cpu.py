"""CPU tests of the BGR subpel temporal filter rule (include/bbme.h, "BGR SUBPEL TEMPORAL FILTER RULE"): the C-ABI exports the
calls; bbme_subpel_temporal_filter_bgr_host follows the rule, which is restated here in vectorised numpy from the header's text and
imported by the GPU tests; the rule's properties (grey frames give the grey subpel rule, 4 x integer grids the integer colour rule,
equal frames stay), validity at every edge of the padded view and every quotient of the two divisions in every channel -- on frame
bytes and on rounded bilinear samples -- carry their answers written out; on noisy colour frames of sub-pixel motion the filtered
middle frame gains in its worst channel what the integer colour rule cannot."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from test_bgr_cpu import SHAPES
from test_gpu_bidirectional import _oracle_fields
from test_interpolation_cpu import extreme_grids, odd_windows, psnr
from test_subpel_interpolation_cpu import _motion_field, fraction_grids, frames_of
from test_subpel_temporal_filter_cpu import (HALF, INTERIOR, NOISE, QUARTER, SIZES, TILES, WHOLE, _texture, edge_grid, fractions_taken,
                                             np_subpel_temporal_filter, sampled_cost_check, sampled_cost_table)
from test_subpel_temporal_filter_cpu import PIPELINE_CASES as GREY_PIPELINE_CASES
from test_temporal_filter_bgr_cpu import in_channel, near_colour_triple, near_grids, np_temporal_filter_bgr
from test_temporal_filter_cpu import (RULE_THRS, S23_THR, STAT_KEYS, THRS, neighbour_sets, np_temporal_filter, s23_table_planes,
                                      s_table_check, s_table_planes, thr_table_expected, thr_table_planes)

NEW_SYMBOLS = ["bbme_subpel_temporal_filter_bgr_host", "bbme_cells_subpel_temporal_filter_bgr_device",
               "bbme_subpel_temporal_filter_bgr_device", "bbme_subpel_temporal_filter_bgr_chain_device",
               "bbme_get_subpel_temporal_filtered_bgr_host", "bbme_subpel_temporal_filter_bgr_stats"]


def np_subpel_temporal_filter_bgr(Cur, P, QP, N, QN, thr, pad_x, pad_y, window=None):
    """The rule of include/bbme.h: every (H, W, 3) frame is read as if zero-padded by (pad_x, pad_y) to H0 x W0; cell (cx, cy) with
    origin o = (2 cx, 2 cy) looks, for each present neighbour X (P with QP, N with QN), at (qx, qy) = Q[cy, cx]: s = o + (qx >> 2,
    qy >> 2), f = (qx & 3, qy & 3); valid when 0 <= s.x, s.x + 2 + (fx != 0) <= W0, 0 <= s.y, s.y + 2 + (fy != 0) <= H0; per channel
    X'[k, j] = ((4 - fx)(4 - fy) T00 + fx (4 - fy) T10 + (4 - fx) fy T01 + fx fy T11 + 8) >> 4 of the taps at s + (j, k) + ...;
    cost_c = sum |C - X'| over the four rounded samples, cost = max over the channels; w = 8 (thr - cost) // thr when valid and
    cost < thr, else 0; S = 8 + wP + wN and every channel of out = (8 C + wP P' + wN N' + S // 2) // S.  Returns (the unpadded
    (H, W, 3) uint8 frame, map uint8 (CH, CW) holding wP | wN << 4, the four statistics over window (cx0, cy0, cw, ch) in cells on
    the padded view) as test_temporal_filter_bgr_cpu.np_temporal_filter_bgr does."""
    H, W = np.asarray(Cur).shape[:2]

    def padded(F):
        return np.pad(np.asarray(F).astype(np.int64), ((pad_y, pad_y), (pad_x, pad_x), (0, 0)))

    Cur = padded(Cur)
    H0, W0 = Cur.shape[:2]
    assert H0 % 2 == 0 and W0 % 2 == 0
    CH, CW = H0 // 2, W0 // 2
    assert (P is None) == (QP is None) and (N is None) == (QN is None) and (P is not None or N is not None)
    cy, cx = np.mgrid[0:CH, 0:CW]
    ox, oy = 2 * cx, 2 * cy
    cell = np.stack([np.stack([Cur[oy + k, ox + j] for j in range(2)]) for k in range(2)])      # [k, j, cy, cx, channel]
    ws, moved = [], []
    for X, Q in ((P, QP), (N, QN)):
        if X is None:
            ws.append(np.zeros((CH, CW), np.int64))
            moved.append(np.zeros((2, 2, CH, CW, 3), np.int64))
            continue
        X = padded(X)
        Q = np.asarray(Q).astype(np.int64)
        qx, qy = Q[..., 0], Q[..., 1]
        fx, fy = qx & 3, qy & 3
        sx, sy = ox + (qx >> 2), oy + (qy >> 2)
        valid = (sx >= 0) & (sx + 2 + (fx != 0) <= W0) & (sy >= 0) & (sy + 2 + (fy != 0) <= H0)

        def tap(dx, dy, weight):                            # a tap of weight 0 is not read: its index is folded into the view
            x = np.where(valid & (weight > 0), sx + dx, 0)
            y = np.where(valid & (weight > 0), sy + dy, 0)
            return weight[..., None] * X[y, x]

        m = np.stack([np.stack([(tap(j, k, (4 - fx) * (4 - fy)) + tap(j + 1, k, fx * (4 - fy)) + tap(j, k + 1, (4 - fx) * fy) +
                                 tap(j + 1, k + 1, fx * fy) + 8) >> 4 for j in range(2)]) for k in range(2)])
        cost = np.abs(cell - m).sum(axis=(0, 1)).max(axis=-1)
        ws.append(np.where(valid & (cost < thr), 8 * (thr - cost) // thr, 0))
        moved.append(m)
    wP, wN = ws
    S = (8 + wP + wN)[..., None]
    pix = (8 * cell + wP[..., None] * moved[0] + wN[..., None] * moved[1] + S // 2) // S
    full = np.empty((H0, W0, 3), np.uint8)
    for k in range(2):
        for j in range(2):
            full[k::2, j::2] = pix[k, j]
    change = np.abs(pix - cell).sum(axis=(0, 1, 4))
    x0, y0, w, h = (0, 0, CW, CH) if window is None else window
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    stats = (int((wP[sl] > 0).sum()), int((wN[sl] > 0).sum()), int((wP[sl] + wN[sl]).sum()), int(change[sl].sum()))
    return np.ascontiguousarray(full[pad_y:pad_y + H, pad_x:pad_x + W]), (wP | wN << 4).astype(np.uint8), stats


def host(bbme, Cur, P, QP, N, QN, thr, pad_x, pad_y, window=None):
    out, wmap, st = bbme.temporal_filter_cells_subpel_bgr(Cur, P, N, QP, QN, thr, pad_x, pad_y, window)
    return out, wmap, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, Cur, P, QP, N, QN, thr, pad_x, pad_y, window=None, what=None):
    exp = np_subpel_temporal_filter_bgr(Cur, P, QP, N, QN, thr, pad_x, pad_y, window)
    got = host(bbme, Cur, P, QP, N, QN, thr, pad_x, pad_y, window)
    tag = (what, thr, P is not None, N is not None, window)
    assert np.array_equal(got[0], exp[0]), tag
    assert np.array_equal(got[1], exp[1]), tag
    assert got[2] == exp[2], tag
    return exp


def near_smooth_triple(w, h, seed):
    """A smooth colour frame (a ramp of its own per channel plus a little noise) and two neighbours near it, so that cells sampled
    between pixels pass at the strengths used"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    Cur = np.stack([(96 + 5 * x + 3 * y), (40 + 2 * x + 7 * y), (200 - 3 * x + 4 * y)], -1) + rng.integers(-6, 7, (h, w, 3))
    Cur = Cur.astype(np.int64) % 256
    P = np.clip(Cur + rng.integers(-5, 6, Cur.shape), 0, 255)
    N = np.clip(Cur + rng.integers(-9, 10, Cur.shape), 0, 255)
    return Cur.astype(np.uint8), P.astype(np.uint8), N.astype(np.uint8)


def flat_triple(w, h, seed):
    """Nearly flat frames: every valid neighbour passes at strength 1021, the zero border included (a cost of at most 4 x 103)"""
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(100, 104, (h, w, 3)).astype(np.uint8) for _ in range(3))


def edge_fraction_grid(H0, W0):
    """A quarter-pel grid in which, for each of the four edges of the H0 x W0 view and each of the 16 fractions (fx, fy), one cell's s
    lies on the last valid position at that edge with that fraction and another one a pixel further out; the other component of
    these cells keeps its own fraction at integer part 0, every other cell is zero -> (grid, [(cx, cy, valid)])."""
    CH, CW = H0 // 2, W0 // 2
    Q = np.zeros((CH, CW, 2), np.int64)
    spots = [(cx, cy) for cy in range(1, CH - 1) for cx in range(1, CW - 1)][::3]      # the other component is valid there
    cells = []
    for axis, n in ((0, W0), (1, H0)):
        for fa in range(4):
            for fo in range(4):
                last = n - 2 - (fa != 0)
                for s, valid in ((0, True), (-1, False), (last, True), (last + 1, False)):
                    cx, cy = spots[len(cells)]
                    c = (cx, cy)[axis]
                    Q[cy, cx, axis] = 4 * s + fa - 8 * c
                    Q[cy, cx, 1 - axis] = fo
                    cells.append((cx, cy, valid))
    assert len(cells) == 128 and np.abs(Q).max() < 32768
    return Q.astype(np.int16), cells


def grey3(a):
    return None if a is None else np.repeat(np.asarray(a)[..., None], 3, axis=2)


def times4(g):
    return None if g is None else (4 * np.asarray(g).astype(np.int32)).astype(np.int16)


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi, sequence
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
        assert "int %s(" % name in header, name
    assert "BGR SUBPEL TEMPORAL FILTER RULE" in header
    assert "The BGR TEMPORAL FILTER RULE stays integer" in header                # true of that rule
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_subpel_temporal_filter_bgr_device(None, d, d, d, 24, d, d, 4, 64, None, d, 24, d, 4, st, None) == inv
    assert L.bbme_subpel_temporal_filter_bgr_device(None, 0, 0, 64, d, 24, None) == inv
    assert L.bbme_subpel_temporal_filter_bgr_chain_device(None, 0, 1, 64, d, 24, 0, None) == inv
    assert L.bbme_get_subpel_temporal_filtered_bgr_host(None, 0, 0, 64, d) == inv
    assert L.bbme_subpel_temporal_filter_bgr_stats(None, 64, None, st) == inv
    assert hasattr(bbme, "temporal_filter_cells_subpel_bgr") and "temporal_filter_cells_subpel_bgr" in bbme.__all__
    for name in ("temporal_filter_subpel_bgr", "temporal_filter_subpel_bgr_stats", "cells_temporal_filter_subpel_bgr_device"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        assert hasattr(cls, "get_frame_filtered_subpel_bgr")
    assert hasattr(bbme.MFChain, "temporal_filter_run_subpel_bgr")
    params = inspect.signature(sequence.denoise_frames).parameters
    assert params["subpel_bgr"].default is False and params["subpel"].default is False
    assert list(params).index("subpel_bgr") == list(params).index("subpel") + 1


def test_context_calls_need_a_device(bbme):
    """Without a GPU no context exists to filter on: there is no CPU fallback behind the context-level calls (the rule on the CPU
    is bbme_subpel_temporal_filter_bgr_host, asked for by name)."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from blockbasedmotionestimation_amd import _capi
    z = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MF(z, z, [32], [16]).temporal_filter_subpel_bgr(64)
    assert e.value.status == _capi.ERR_HIP and "no CPU fallback" in e.value.message


def test_grey_frames_with_subpel_bgr_are_a_value_error(bbme):
    from blockbasedmotionestimation_amd import sequence
    z = np.zeros((64, 64), np.uint8)
    with pytest.raises(ValueError):
        sequence.denoise_frames([z, z, z], [32], [16], 64, subpel_bgr=True)


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
        return L.bbme_subpel_temporal_filter_bgr_host(p, c, n, w, h, px, py, gp, gn, thr, win, o, m, t)

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
        bbme.temporal_filter_cells_subpel_bgr(img, img, None, g[:, :4], None, 64, px, py)
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_subpel_bgr(img, img, None, None, None, 64, px, py)    # a frame without its grid
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.temporal_filter_cells_subpel_bgr(img, img, None, g, None, 64, 0, py)        # 14 x 12: the grid is of another geometry
    assert e.value.status == inv


@pytest.mark.parametrize("shape", list(SHAPES))
def test_host_rule_equals_numpy_on_every_fraction(bbme, shape):
    """Grids of up to 14 quarter pels plus far vectors, both neighbours and each alone, RULE_THRS plus 8 and 24, full and odd
    windows: frame, map and statistics; over the seeds every (fx, fy) class is taken by both neighbours."""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    CH, CW = H0 // 2, W0 // 2
    wins = odd_windows(CH, CW)
    seen = [set(), set()]
    weights = set()
    n = 0
    for seed in range(2):
        Cur, P, N = near_smooth_triple(w, h, 10 * h + w + seed)
        qp, qn = fraction_grids(H0, W0, 100 * W0 + H0 + seed)
        for thr in RULE_THRS + (8, 24):
            for p, a, q, b in neighbour_sets(P, qp, N, qn):
                exp = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, px, py, wins[n % len(wins)], (shape, seed))
                n += 1
                if p is not None and q is not None and thr >= 255:
                    fp, fn = fractions_taken(exp[1], qp, qn)
                    seen[0] |= fp
                    seen[1] |= fn
                    weights |= set(np.unique(exp[1] & 0x0f).tolist()) | set(np.unique(exp[1] >> 4).tolist())
    every = {(a, b) for a in range(4) for b in range(4)}
    assert seen[0] == every and seen[1] == every
    assert weights >= set(range(8))                         # 8 needs a cost of 0: test_property_3
    # random frames: most cells fail, the few that pass blend bytes from anywhere
    Cur, P, N = near_colour_triple(w, h, 7 * w + h)
    qp, qn = fraction_grids(H0, W0, 3 * W0 + H0, reach=5)
    for thr in (64, 1021):
        assert_host_equals_numpy(bbme, Cur, P, qp, N, qn, thr, px, py, wins[1], shape)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_validity_at_every_edge_of_the_padded_view(bbme, shape):
    """A cell whose s lies on the last valid position of the PADDED view takes its neighbour -- with pads > 0 its taps then lie in
    the zero border, with odd pads the cell straddles the frame's edge --; one a quarter pel (f = 0) or a pixel (f != 0) further
    out has weight 0 and keeps C's pixels.  The frames are nearly flat, so that every valid cell passes at strength 1021."""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    Cur, P, N = flat_triple(w, h, H0 + W0)
    Q, cells = edge_grid(H0, W0)
    assert sum(v for _, _, v in cells) == 16 and len(cells) == 32
    padC = np.pad(Cur, ((py, py), (px, px), (0, 0)))
    for p, a, q, b in neighbour_sets(P, Q, N, Q):
        out, wmap, _ = assert_host_equals_numpy(bbme, Cur, p, a, q, b, 1021, px, py, None, shape)
        full = np.pad(out, ((py, py), (px, px), (0, 0)))
        for cx, cy, valid in cells:
            wp, wn = wmap[cy, cx] & 0x0f, wmap[cy, cx] >> 4
            assert (wp > 0) == (valid and p is not None) and (wn > 0) == (valid and q is not None), (cx, cy, valid)
            if not valid:
                assert np.array_equal(full[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2], padC[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_fraction_at_every_edge(bbme, shape):
    """All 16 fractions on the last valid position of each edge of the padded view and a pixel past it"""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    Cur, P, N = flat_triple(w, h, 3 * H0 + W0)
    Q, cells = edge_fraction_grid(H0, W0)
    for p, a, q, b in neighbour_sets(P, Q, N, Q):
        _, wmap, _ = assert_host_equals_numpy(bbme, Cur, p, a, q, b, 1021, px, py, None, shape)
        for cx, cy, valid in cells:
            wp, wn = wmap[cy, cx] & 0x0f, wmap[cy, cx] >> 4
            assert (wp > 0) == (valid and p is not None) and (wn > 0) == (valid and q is not None), (cx, cy, valid)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_int16_extremes_leave_the_frame_alone(bbme, shape):
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    rng = np.random.default_rng(11 * w + h)
    Cur, P, N = (rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3))
    qp, qn = extreme_grids(H0 // 2, W0 // 2, rng)
    for thr in RULE_THRS:
        for p, a, q, b in neighbour_sets(P, qp, N, qn):
            out, wmap, st = assert_host_equals_numpy(bbme, Cur, p, a, q, b, thr, px, py, None)
            assert np.array_equal(out, Cur) and not wmap.any() and st == (0, 0, 0, 0)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_property_1_grey_frames_give_the_grey_subpel_rule(bbme, shape):
    """B = G = R: every channel is the unpadded window of the SUBPEL TEMPORAL FILTER RULE's result (its numpy restatement) on the
    zero-padded plane, the map and the first three statistics are equal and the fourth is three times the grey one."""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    CH, CW = H0 // 2, W0 // 2
    Cur, P, N = (f[..., 0] for f in near_smooth_triple(w, h, 5 * w + h))
    qp, qn = fraction_grids(H0, W0, 9 * W0 + H0)
    wins = odd_windows(CH, CW)
    pad = lambda f: None if f is None else bbme.pad_zero(f, px, py)
    taken = 0
    for n, thr in enumerate(RULE_THRS):
        win = wins[n % len(wins)]
        for p, a, q, b in neighbour_sets(P, qp, N, qn):
            eo, em, es = np_subpel_temporal_filter(pad(Cur), pad(p), a, pad(q), b, thr, win)
            out, wmap, st = host(bbme, grey3(Cur), grey3(p), a, grey3(q), b, thr, px, py, win)
            for k in range(3):
                assert np.array_equal(out[..., k], eo[py:py + h, px:px + w]), (shape, thr, k)
            assert np.array_equal(wmap, em)
            assert st == (es[0], es[1], es[2], 3 * es[3])
            taken += es[2]
    assert taken > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_property_2_four_times_integer_grids_give_the_integer_colour_rule(bbme, shape):
    """QP = 4 GP, QN = 4 GN: frame, map and statistics are bbme.temporal_filter_cells_bgr's on GP, GN, bit for bit"""
    w, h, _, _ = shape
    W0, H0, px, py = SHAPES[shape]
    CH, CW = H0 // 2, W0 // 2
    Cur, P, N = near_colour_triple(w, h, 7 * w + h)
    rng = np.random.default_rng(3 * w + h)
    gp, gn = near_grids(CH, CW, rng)
    big = rng.random((CH, CW)) < 0.1                        # vectors that leave the view, still inside int16 when multiplied by 4
    gp[big] = (W0, -3)
    gn[big] = (-2, -H0)
    wins = odd_windows(CH, CW)
    taken = 0
    for n, thr in enumerate(RULE_THRS + (8, 24)):
        for k, (p, a, q, b) in enumerate(neighbour_sets(P, gp, N, gn)):
            win = wins[(n + k) % len(wins)]
            old = bbme.temporal_filter_cells_bgr(Cur, p, q, a, b, thr, px, py, win)
            new = bbme.temporal_filter_cells_subpel_bgr(Cur, p, q, times4(a), times4(b), thr, px, py, win)
            assert np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]) and old[2] == new[2], (shape, thr, k)
            exp = np_temporal_filter_bgr(Cur, p, a, q, b, thr, px, py, win)
            assert np.array_equal(new[0], exp[0]) and np.array_equal(new[1], exp[1])
            taken += old[2]["prev_cells"] + old[2]["next_cells"]
    assert taken > 0


def test_property_3_equal_frames_and_zero_grids_keep_the_frame(bbme):
    rng = np.random.default_rng(31)
    h, w, px, py = 38, 54, 1, 1
    Cur = rng.integers(1, 256, (h, w, 3)).astype(np.uint8)
    CH, CW = (h + 2 * py) // 2, (w + 2 * px) // 2
    z = np.zeros((CH, CW, 2), np.int16)
    cells = CH * CW
    for thr in THRS:
        out, wmap, st = host(bbme, Cur, Cur, z, Cur, z, thr, px, py)
        assert np.array_equal(out, Cur) and (wmap == 0x88).all() and st == (cells, cells, 16 * cells, 0)
        out, wmap, st = host(bbme, Cur, None, None, Cur, z, thr, px, py)
        assert np.array_equal(out, Cur) and (wmap == 0x80).all() and st == (0, cells, 8 * cells, 0)
        out, wmap, st = host(bbme, Cur, Cur, z, None, None, thr, px, py)
        assert np.array_equal(out, Cur) and (wmap == 0x08).all() and st == (cells, 0, 8 * cells, 0)


def division_tables_in_channel(filt, k):
    """The grey tests' tables (every cost 0..1020 at the eight strengths; every S = 9..23 with every residue class) in channel k
    through `filt`(Cur, P, QP, N, QN, thr) -> (out, map, ...) with zero quarter-pel grids, the two other channels carrying C's own
    values in all three frames (cost 0: cheaper): channel k is the grey table's output."""
    Cur, N, cost = thr_table_planes()
    z = np.zeros(cost.shape + (2,), np.int16)
    rest = (np.arange(Cur.size).reshape(Cur.shape) * 7 % 251).astype(np.uint8)
    fC, fN = in_channel(Cur, k, rest), in_channel(N, k, rest)
    for thr in THRS:
        exp = thr_table_expected(cost, thr)
        out, wmap = filt(fC, None, None, fN, z, thr)[:2]
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
        out, wmap = filt(in_channel(Cur, k, rest), in_channel(P, k, rest), z, in_channel(N, k, rest), z, thr)[:2]
        s_table_check(Cur, P, N, expect_w, out[..., k], wmap, pairs=pairs, ends=ends)
        exp = np_subpel_temporal_filter_bgr(in_channel(Cur, k, rest), in_channel(P, k, rest), z, in_channel(N, k, rest), z, thr, 0, 0)
        assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1])


def sampled_costs_in_channel(filt, k, thr):
    """sampled_cost_table() (every cost 0..1020 from ROUNDED half-pel samples) in channel k through `filt`, as the next neighbour
    and as the previous one; the two other channels are one constant in all frames, whose samples are that constant: cost 0."""
    Cur, X, grid, cost = sampled_cost_table()
    rest = np.full(Cur.shape, 77, np.uint8)
    fC, fX = in_channel(Cur, k, rest), in_channel(X, k, rest)
    for P, QP, N, QN, shift in ((None, None, fX, grid, 4), (fX, grid, None, None, 0)):
        out, wmap = filt(fC, P, QP, N, QN, thr)[:2]
        exp = np_subpel_temporal_filter_bgr(fC, P, QP, N, QN, thr, 0, 0)
        assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1])
        sampled_cost_check(cost, thr, out[..., k], (wmap >> shift) & 0x0f)
        for o in range(3):
            if o != k:
                assert (out[..., o] == 77).all()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_divisions_are_exact_in_every_channel(bbme, k):
    division_tables_in_channel(lambda Cur, P, QP, N, QN, thr: host(bbme, Cur, P, QP, N, QN, thr, 0, 0), k)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_division_on_sampled_costs_in_every_channel(bbme, k):
    for thr in (1, 64, 1021):
        sampled_costs_in_channel(lambda Cur, P, QP, N, QN, thr: host(bbme, Cur, P, QP, N, QN, thr, 0, 0), k, thr)


# ---- quality: the grey test's setup with one independent texture per channel ----------------------------------------------------

def noisy_subpel_bgr_frames(w, h, size, tiles, sigma):
    """Frames 0, 1, 2 in colour: channel c's clean frames are frames_of(_texture(w, h, 100 + size + 50 c), w, h, 2 motion), stacked
    B, G, R; ONE default_rng(100 + size + 2) draws normal(0, sigma, (h, w, 3)) on frames 0, 1, 2 in this order -> (clean, noisy,
    quarter-pel grid from frame 1 into frame 2)"""
    mo = _motion_field(w, h, tiles)
    chans = [frames_of(_texture(w, h, 100 + size + 50 * c), w, h, 2 * mo) for c in range(3)]
    clean = [np.stack([chans[c][k] for c in range(3)], -1) for k in range(3)]
    noise = np.random.default_rng(100 + size + 2)
    noisy = [np.clip(np.rint(f + noise.normal(0.0, sigma, (h, w, 3))), 0, 255).astype(np.uint8) for f in clean]
    return clean, noisy, mo[::2, ::2].astype(np.int64)


def worst_channel_gain(frame, noisy, clean):
    k = (slice(INTERIOR, -INTERIOR), slice(INTERIOR, -INTERIOR))
    return min(psnr(frame[k][..., c], clean[k][..., c]) - psnr(noisy[k][..., c], clean[k][..., c]) for c in range(3))


@pytest.mark.parametrize("noise", NOISE)
@pytest.mark.parametrize("size", range(len(SIZES)))
@pytest.mark.parametrize("case", WHOLE + HALF + QUARTER + TILES)
def test_quality_against_the_clean_middle_frame(bbme, capsys, case, size, noise):
    """The PSNR gain of the filtered middle frame over the noisy one, worst channel, interior of 16 pixels, pads 0: the new rule on
    the true quarter-pel grids q and -q against the integer BGR rule on (q + 2) >> 2 and its negative.  The floors are the grey
    test's.  Measured (worst channel over both sizes and the three noise levels, two-sided / one-sided, dB):
        motion                     integer BGR rule                     this rule                          smallest difference
        WHOLE                      +4.33..+4.67 / +2.66..+2.82          the same frames                    0
        HALF                       +2.05..+4.50 / +0.26..+2.38          +5.23..+6.67 / +3.56..+4.19        +2.15 / +1.77
        QUARTER                    +4.00..+4.56 / +1.42..+2.65          +5.33..+6.18 / +3.45..+3.88        +1.33 / +1.19
        TILES                      +2.00..+4.28 / +0.29..+2.05          +5.07..+6.35 / +3.09..+3.76        +2.06 / +1.59
    """
    w, h = SIZES[size]
    sigma, thr = noise
    tiles = (case,) if isinstance(case[0], int) else case
    clean, (f0, f1, f2), q = noisy_subpel_bgr_frames(w, h, size, tiles, sigma)
    q_next, q_prev = q.astype(np.int16), (-q).astype(np.int16)
    i_next = ((q + 2) >> 2).astype(np.int16)
    i_prev = (-i_next).astype(np.int16)
    new2 = assert_host_equals_numpy(bbme, f1, f0, q_prev, f2, q_next, thr, 0, 0, None, case)
    new1 = assert_host_equals_numpy(bbme, f1, None, None, f2, q_next, thr, 0, 0, None, case)
    old2 = bbme.temporal_filter_cells_bgr(f1, f0, f2, i_prev, i_next, thr)
    old1 = bbme.temporal_filter_cells_bgr(f1, None, f2, None, i_next, thr)
    g = {name: worst_channel_gain(r[0], f1, clean[1]) for name, r in (("new2", new2), ("new1", new1), ("old2", old2), ("old1", old1))}
    with capsys.disabled():
        print("\nbgr subpel temporal filter %dx%d motion %s sigma %d strength %d, worst channel: integer BGR rule two-sided %+.2f dB "
              "one-sided %+.2f dB | quarter-pel colour rule two-sided %+.2f dB one-sided %+.2f dB | weights %s"
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


# (tiles, sigma, strength): the statistics of the integer colour route and of the quarter-pel colour route, from the first run
PIPELINE_CASES = {
    (((10, 6),), 3, 64): ((2733, 2602, 19756, 66143), (2816, 2730, 29608, 57088)),
    (((10, 6),), 6, 128): ((2997, 2921, 27392, 131131), (3005, 2945, 31749, 113920)),
    (((10, 6),), 10, 256): ((3065, 3069, 32776, 217749), (3067, 3070, 35018, 197564)),
    (((2, 2), (10, 6), (14, -10), (-6, 2)), 3, 64): ((2678, 2777, 19929, 64662), (2805, 2856, 29253, 58423)),
    (((2, 2), (10, 6), (14, -10), (-6, 2)), 6, 128): ((2988, 2973, 27677, 128971), (2996, 2988, 31794, 115787)),
    (((2, 2), (10, 6), (14, -10), (-6, 2)), 10, 256): ((3050, 3064, 32975, 214988), (3052, 3067, 35036, 198300)),
}
assert list(PIPELINE_CASES) == list(GREY_PIPELINE_CASES)


@pytest.mark.parametrize("case", list(GREY_PIPELINE_CASES))
def test_pipeline_on_the_oracles_fields(bbme, oracle, capsys, case):
    """The whole route on the CPU in colour, the noise entering estimate and refinement: the oracle's fields (f1, f0) and (f1, f2)
    on the LUMA of the noisy frames, refined by bbme.subpel_cells on the padded luma planes, then the new rule on the colour
    frames; against bbme.temporal_filter_cells_bgr on the same oracle fields.  The new route may not be worse than the integer
    route by more than 0.5 dB (the grey test's tolerance for noise entering the refinement).  Measured (integer route / quarter-pel
    route, worst channel's gain over the noisy frame in dB, sigma 3, 6, 10): motion (10, 6) +0.93 / +5.10, +2.62 / +5.83,
    +3.83 / +5.95; the half-pel tiles +1.25 / +4.64, +2.89 / +5.39, +3.97 / +5.63: the route loses nowhere."""
    tiles, sigma, thr = case
    w, h, search, block = 128, 96, [48, 48], [16, 16]
    clean, (f0, f1, f2), _ = noisy_subpel_bgr_frames(w, h, 0, tiles, sigma)
    y0, y1, y2 = (bbme.bgr_to_gray(f) for f in (f0, f1, f2))
    _, to_prev = _oracle_fields(bbme, oracle, y1, y0, search, block)
    _, to_next = _oracle_fields(bbme, oracle, y1, y2, search, block)
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    P, Cur, N = (bbme.pad_zero(y, px, py) for y in (y0, y1, y2))
    q_prev, _ = bbme.subpel_cells(Cur, P, to_prev)
    q_next, _ = bbme.subpel_cells(Cur, N, to_next)
    old, _, st_old = bbme.temporal_filter_cells_bgr(f1, f0, f2, to_prev, to_next, thr, px, py)
    new, _, st_new = assert_host_equals_numpy(bbme, f1, f0, q_prev, f2, q_next, thr, px, py, None, "pipeline")
    st_old = tuple(st_old[k] for k in STAT_KEYS)
    g_old, g_new = worst_channel_gain(old, f1, clean[1]), worst_channel_gain(new, f1, clean[1])
    with capsys.disabled():
        print("\nbgr subpel temporal filter pipeline %dx%d motion %s sigma %d strength %d, worst channel: integer route %+.2f dB %s | "
              "quarter-pel route %+.2f dB %s" % (w, h, tiles, sigma, thr, g_old, st_old, g_new, st_new))
    assert g_new >= g_old - 0.5, (g_old, g_new)
    assert (st_old, st_new) == PIPELINE_CASES[case]
