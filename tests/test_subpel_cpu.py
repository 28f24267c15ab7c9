"""CPU tests of the subpel rule (include/bbme.h, "SUBPEL RULE"): the C-ABI exports the subpel calls; bbme_subpel_host follows the
rule, which is restated here in vectorised numpy from the header's text (the four-term sample, not the separable form the C code
and the kernel use) and imported by the GPU tests; planted quarter-pel shifts are recovered exactly; on the Venus pair the refined
field of the oracle's integer estimate comes within reach of the reference's x4 pipeline at a sixteenth of the pixels."""
import ctypes as C
import os

import numpy as np
import pytest

NEW_SYMBOLS = ["bbme_subpel_host", "bbme_cells_subpel_device", "bbme_subpel_device", "bbme_get_subpel_cells_host",
               "bbme_subpel_stats", "bbme_get_subpel_flow_host"]

STAT_KEYS = ("valid", "moved", "cost_integer", "cost_refined")
ORDER = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


class Rule:
    """The rule on one plane pair and grid: validity, cost(q) of every cell for a per-cell q, and the search."""

    def __init__(self, I1, I2, G):
        self.I1 = np.asarray(I1).astype(np.int64)
        self.I2 = np.asarray(I2).astype(np.int64)
        self.G = np.asarray(G).astype(np.int64)
        H0, W0 = self.I1.shape
        self.CH, self.CW = H0 // 2, W0 // 2
        cy, cx = np.mgrid[0:self.CH, 0:self.CW]
        ax, ay = 2 * cx - 3, 2 * cy - 3
        bx, by = ax + self.G[..., 0], ay + self.G[..., 1]
        self.valid = ((0 <= ax) & (ax + 8 <= W0) & (0 <= ay) & (ay + 8 <= H0) &
                      (2 <= bx) & (bx + 10 <= W0) & (2 <= by) & (by + 10 <= H0))
        # invalid cells are evaluated somewhere harmless and masked afterwards
        self.ax, self.ay = np.where(self.valid, ax, 0), np.where(self.valid, ay, 0)
        self.bx, self.by = np.where(self.valid, bx, 2), np.where(self.valid, by, 2)

    def cost(self, qx, qy):
        """cost(q) per cell, q = (qx, qy) scalars or (CH, CW) arrays"""
        qx = np.broadcast_to(np.asarray(qx, np.int64), (self.CH, self.CW))
        qy = np.broadcast_to(np.asarray(qy, np.int64), (self.CH, self.CW))
        ix, iy, fx, fy = qx >> 2, qy >> 2, qx & 3, qy & 3
        total = np.zeros((self.CH, self.CW), np.int64)
        for i in range(8):
            for j in range(8):
                y, x = self.by + i + iy, self.bx + j + ix
                P00, P10, P01, P11 = self.I2[y, x], self.I2[y, x + 1], self.I2[y + 1, x], self.I2[y + 1, x + 1]
                s = ((4 - fx) * (4 - fy) * P00 + fx * (4 - fy) * P10 + (4 - fx) * fy * P01 + fx * fy * P11 + 8) >> 4
                total += np.abs(self.I1[self.ay + i, self.ax + j] - s)
        return total

    def search(self):
        """-> (qx, qy, cost(0, 0), best) per cell; q = 0 on invalid cells"""
        zero = np.zeros((self.CH, self.CW), np.int64)
        qx, qy = zero.copy(), zero.copy()
        cost0 = self.cost(0, 0)
        best = cost0.copy()
        for s in (2, 1):
            c_x, c_y = qx.copy(), qy.copy()
            for dx, dy in ORDER:
                k = self.cost(c_x + s * dx, c_y + s * dy)
                better = k < best
                best = np.where(better, k, best)
                qx = np.where(better, c_x + s * dx, qx)
                qy = np.where(better, c_y + s * dy, qy)
        return np.where(self.valid, qx, 0), np.where(self.valid, qy, 0), cost0, best


def np_subpel(I1, I2, G, window=None):
    """The rule of include/bbme.h -> (quarter-pel grid int16 (CH, CW, 2), (valid cells, cells with q != 0, sum of cost(0, 0), sum
    of best) over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    r = Rule(I1, I2, G)
    qx, qy, cost0, best = r.search()
    out = np.clip(4 * r.G + np.stack([qx, qy], -1), -32768, 32767).astype(np.int16)
    if window is None:
        window = (0, 0, r.CW, r.CH)
    x0, y0, w, h = window
    sl = (slice(y0, y0 + h), slice(x0, x0 + w))
    v = r.valid[sl]
    stats = (int(v.sum()), int((v & ((qx[sl] != 0) | (qy[sl] != 0))).sum()), int(cost0[sl][v].sum()), int(best[sl][v].sum()))
    return out, stats


def host_subpel(bbme, I1, I2, G, window=None):
    out, st = bbme.subpel_cells(I1, I2, G, window)
    return out, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, I1, I2, G, window=None, what=None):
    exp = np_subpel(I1, I2, G, window)
    got = host_subpel(bbme, I1, I2, G, window)
    assert np.array_equal(got[0], exp[0]), (what, window)
    assert got[1] == exp[1], (what, window, got[1], exp[1])
    return exp


def texture(bbme, w, h, seed):
    return bbme.synth_pair(w, h, seed, max_motion=0, noise=0)[0]


def random_case(bbme, w, h, seed, spread=5):
    """Two textured planes, the second roughly the first moved by a smooth field, and a grid near that field"""
    rng = np.random.default_rng(seed)
    f1, f2, motion = bbme.synth_pair(w, h, seed, max_motion=spread, tiles=3)
    G = motion[::2, ::2].astype(np.int16) + rng.integers(-1, 2, size=(h // 2, w // 2, 2)).astype(np.int16)
    return f1, f2, G


def boundary_vectors(w, h, cx, cy):
    """For cell (cx, cy): the eight vectors that put b on a validity bound (valid) and the eight one past it (invalid)"""
    ax, ay = 2 * cx - 3, 2 * cy - 3
    on = [(2 - ax, 0), (w - 10 - ax, 0), (0, 2 - ay), (0, h - 10 - ay),
          (2 - ax, 2 - ay), (w - 10 - ax, h - 10 - ay), (2 - ax, h - 10 - ay), (w - 10 - ax, 2 - ay)]
    past = [(1 - ax, 0), (w - 9 - ax, 0), (0, 1 - ay), (0, h - 9 - ay),
            (1 - ax, 2 - ay), (w - 9 - ax, h - 10 - ay), (2 - ax, h - 9 - ay), (w - 10 - ax, 1 - ay)]
    return on, past


def boundary_grid(w, h, seed):
    """A grid whose interior cells carry, in turn, the boundary vectors of their own position -> (grid, [(cx, cy, valid)])"""
    rng = np.random.default_rng(seed)
    G = rng.integers(-2, 3, size=(h // 2, w // 2, 2)).astype(np.int16)
    cells = []
    k = 0
    for cy in range(3, h // 2 - 4, 2):
        for cx in range(3, w // 2 - 4, 2):
            on, past = boundary_vectors(w, h, cx, cy)
            v, ok = ((on + past)[k % 16], k % 16 < 8)
            G[cy, cx] = v
            cells.append((cx, cy, ok))
            k += 1
    assert k >= 16
    return G, cells


def extreme_grid(w, h, seed):
    rng = np.random.default_rng(seed)
    G = rng.integers(-3, 4, size=(h // 2, w // 2, 2)).astype(np.int16)
    ext = np.array([-32768, 32767, -8192, 8191, -8193, 8192, 0], np.int16)
    pick = rng.random((h // 2, w // 2)) < 0.3
    G[pick] = ext[rng.integers(0, len(ext), size=(int(pick.sum()), 2))]
    return G


SIZES = ((70, 50), (64, 48))


@pytest.mark.parametrize("w,h", SIZES)
def test_host_rule_equals_numpy_on_random_planes(bbme, w, h):
    for seed in (1, 2):
        f1, f2, G = random_case(bbme, w, h, 100 * seed + w)
        _, st = assert_host_equals_numpy(bbme, f1, f2, G, None, "random")
        assert st[0] > 0.5 * G.shape[0] * G.shape[1] and 0 < st[1] <= st[0] and st[3] < st[2]
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 256, size=(2, h, w)).astype(np.uint8)              # white noise: the costs reach their upper range
    G = rng.integers(-12, 13, size=(h // 2, w // 2, 2)).astype(np.int16)
    assert_host_equals_numpy(bbme, a, b, G, None, "noise")
    a[:], b[:] = 0, 255                                                       # every cost at its ceiling 16320
    exp, st = assert_host_equals_numpy(bbme, a, b, np.zeros_like(G), None, "ceiling")
    assert st[2] == st[3] == 16320 * st[0] and st[1] == 0


@pytest.mark.parametrize("w,h", SIZES)
def test_windowed_statistics(bbme, w, h):
    f1, f2, G = random_case(bbme, w, h, 31)
    cw, ch = w // 2, h // 2
    total = np.zeros(4, np.int64)
    for win in ((0, 0, cw, ch), (0, 0, 5, ch), (5, 0, cw - 5, 7), (5, 7, cw - 5, ch - 7), (cw - 1, ch - 1, 1, 1), (3, 2, 1, 1)):
        _, st = assert_host_equals_numpy(bbme, f1, f2, G, win, "window")
        if win in ((0, 0, 5, ch), (5, 0, cw - 5, 7), (5, 7, cw - 5, ch - 7)):
            total += st
    assert tuple(total) == np_subpel(f1, f2, G)[1]                            # the three windows tile the grid
    _, st = bbme.subpel_cells(f1, f2, G)                                      # the statistics do not need the grid written
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    s4 = (C.c_ulonglong * 4)()
    assert L.bbme_subpel_host(f1.ctypes.data, f2.ctypes.data, w, h, G.ctypes.data, None, None, s4) == 0
    assert tuple(s4) == tuple(st[k] for k in STAT_KEYS)


@pytest.mark.parametrize("w,h", SIZES)
def test_validity_bounds_and_extreme_vectors(bbme, w, h):
    f1, f2, _ = random_case(bbme, w, h, 5)
    G, cells = boundary_grid(w, h, 9)
    out, _ = assert_host_equals_numpy(bbme, f1, f2, G, None, "bounds")
    r = Rule(f1, f2, G)
    for cx, cy, ok in cells:
        assert bool(r.valid[cy, cx]) == ok, (cx, cy, ok)
        _, st = host_subpel(bbme, f1, f2, G, (cx, cy, 1, 1))
        assert st[0] == int(ok), (cx, cy, ok)
        if not ok:
            assert np.array_equal(out[cy, cx], 4 * G[cy, cx])
    # the window's own bounds: a.x = 2 cx - 3 >= 0 from cx = 2 on, a.x + 8 <= W0 up to 2 cx + 5 <= W0
    Z = np.zeros((h // 2, w // 2, 2), np.int16)
    r = Rule(f1, f2, Z)
    vx = [cx for cx in range(w // 2) if r.valid[h // 4, cx]]
    vy = [cy for cy in range(h // 2) if r.valid[cy, w // 4]]
    assert (vx[0], vx[-1]) == (3, (w - 7) // 2) and (vy[0], vy[-1]) == (3, (h - 7) // 2)     # b = a: b's bounds bind first
    assert_host_equals_numpy(bbme, f1, f2, Z, None, "zero")
    E = extreme_grid(w, h, 11)
    out, _ = assert_host_equals_numpy(bbme, f1, f2, E, None, "extreme")
    assert out.min() == -32768 and out.max() == 32767                         # saturated, on invalid cells only
    big = (np.abs(E.astype(np.int64)) >= 8192).any(-1)
    assert not Rule(f1, f2, E).valid[big].any()


def test_flat_planes_keep_q_zero(bbme):
    for w, h in SIZES:
        for a, b in ((0, 0), (255, 255), (10, 200), (200, 10)):
            I1, I2 = np.full((h, w), a, np.uint8), np.full((h, w), b, np.uint8)
            G = np.random.default_rng(a + b).integers(-3, 4, size=(h // 2, w // 2, 2)).astype(np.int16)
            out, st = assert_host_equals_numpy(bbme, I1, I2, G, None, "flat")
            assert np.array_equal(out, 4 * G) and st[1] == 0 and st[2] == st[3] == 64 * abs(a - b) * st[0]


def test_ties_go_to_the_earlier_candidate(bbme):
    """Planes mirrored about the centre of one cell's window (W0 / 2 odd: the centre cell's window is x = W0 / 2 - 4 .. W0 / 2 + 3):
    there cost(-qx, qy) = cost(qx, qy) for every q, so whenever the half-pel stage's best has qx != 0 its mirror ties with it, and
    the rule takes the one visited first: qx = -2."""
    w, h = 70, 50
    cx = (w // 2 - 1) // 2
    found = 0
    for seed in range(10):
        t1, t2 = texture(bbme, w, h, 300 + seed), texture(bbme, w, h, 400 + seed)
        I2 = ((t2.astype(np.int64) + t2[:, ::-1]) // 2).astype(np.uint8)
        I1 = ((t1.astype(np.int64) + t1[:, ::-1] + t2 + t2[:, ::-1]) // 4).astype(np.uint8)
        G = np.zeros((h // 2, w // 2, 2), np.int16)
        r = Rule(I1, I2, G)
        for q in ((2, 0), (1, 3), (3, -2), (2, 2)):
            assert np.array_equal(r.cost(q[0], q[1])[3:-4, cx], r.cost(-q[0], q[1])[3:-4, cx])
        stage = np.stack([r.cost(2 * dx, 2 * dy) for dx, dy in ORDER])        # the half-pel stage
        cost0 = r.cost(0, 0)
        out, _ = assert_host_equals_numpy(bbme, I1, I2, G, None, "mirror")
        for cy in range(3, h // 2 - 4):
            k = int(stage[:, cy, cx].argmin())                                # the first of the smallest: the rule's winner
            if stage[k, cy, cx] < cost0[cy, cx] and ORDER[k][0] != 0:
                assert ORDER[k][0] == -1 and stage[k, cy, cx] == stage[ORDER.index((1, ORDER[k][1])), cy, cx]
                assert out[cy, cx, 0] in (-3, -2, -1), (seed, cy, out[cy, cx])  # a quarter-pel step around qx = -2
                found += 1
    assert found >= 5, found


PLANT_W, PLANT_H = 64, 48


def planted_texture(bbme, seed):
    """Every third pixel of a synth_pair texture (max_motion=0, noise=0) of three times the size.  The texture as it comes has
    features about as large as the rule's 8 x 8 window (three 5 x 5 box blurs): a tenth of the windows then have next to no
    gradient in one direction, the half-pel stage slides two quarter-pels along it for nothing, and the quarter-pel stage can only
    come back one -- the restatement alone misses a planted q0 with one odd component on 2 to 15 % of the cells there (seeds 77,
    1, 2, 3).  At a third of the feature size every window has gradient in both directions, and the restatement recovers all 49
    shifts on every valid cell (seeds 77, 1, 2); subsampled by two it still misses some 20 cells of 49 x 468."""
    return np.ascontiguousarray(texture(bbme, 3 * PLANT_W, 3 * PLANT_H, seed)[::3, ::3])


def planted_pair(bbme, q0, seed=77):
    """I2 a texture, I1 its exact sample at the constant offset q0 wherever the sample's four pixels exist (0 elsewhere)"""
    I2 = planted_texture(bbme, seed).astype(np.int64)
    qx, qy = q0
    ix, iy, fx, fy = qx >> 2, qy >> 2, qx & 3, qy & 3
    I1 = np.zeros_like(I2)
    ys, xs = np.mgrid[1:PLANT_H - 1, 1:PLANT_W - 1]
    y, x = ys + iy, xs + ix
    I1[ys, xs] = ((4 - fx) * (4 - fy) * I2[y, x] + fx * (4 - fy) * I2[y, x + 1] + (4 - fx) * fy * I2[y + 1, x] +
                  fx * fy * I2[y + 1, x + 1] + 8) >> 4
    return I1.astype(np.uint8), I2.astype(np.uint8)


@pytest.mark.parametrize("qy", range(-3, 4))
def test_planted_shifts_are_recovered(bbme, qy):
    G = np.zeros((PLANT_H // 2, PLANT_W // 2, 2), np.int16)
    for qx in range(-3, 4):
        I1, I2 = planted_pair(bbme, (qx, qy))
        r = Rule(I1, I2, G)
        assert r.valid[3:-3, 3:-3].all() and r.valid.sum() == r.valid[3:-3, 3:-3].size
        assert (r.cost(qx, qy)[r.valid] == 0).all()
        exp, _ = np_subpel(I1, I2, G)                                         # the walk itself finds the planted optimum ...
        assert (exp[r.valid] == (qx, qy)).all(), (qx, qy)
        got, st = host_subpel(bbme, I1, I2, G)                                # ... and so does the library
        assert (got[r.valid] == (qx, qy)).all() and (got[~r.valid] == 0).all(), (qx, qy)
        assert st[0] == r.valid.sum() and st[3] == 0 and st[1] == (st[0] if (qx, qy) != (0, 0) else 0)


def cells_to_field(q4, pad_x, pad_y, w, h, div):
    """The unpadded w x h field of a cell grid: pixel (x, y) = cell((pad_y + y) >> 1, (pad_x + x) >> 1) / div"""
    ys, xs = np.mgrid[0:h, 0:w]
    return (q4[(pad_y + ys) >> 1, (pad_x + xs) >> 1].astype(np.float32) / np.float32(div)).astype(np.float32)


def test_quality_on_the_venus_pair(bbme, oracle, venus_flo, capsys):
    """The pair of bench.py (a texture warped by Venus flow10.flo, 420 x 380) at its own resolution, search [16] * 3, block [8] * 3:
    the oracle's integer field, the same refined, and the reference's x4 pipeline ([64] * 4, [32] * 4 on the frames enlarged x4,
    every 4th pixel / 4), each as Flow::CalculateMSE against the ground truth.  Measured when the rule was chosen, in float64:
    0.3461, 0.1865 and 0.1690 px with 94.3 % of the padded plane's cells valid."""
    flow = bbme.Flow()
    gt = flow.ReadFlowFile(venus_flo)
    h, w = gt.shape[:2]
    f1, f2 = bbme.warp_pair_from_flow(gt)
    omf = oracle.OracleMF(f1, f2, [16] * 3, [8] * 3)
    field = omf.calc_motion_block_matching()
    p1, p2 = omf.image(0, 1).copy(), omf.image(0, 2).copy()
    px, py = omf.padding_x, omf.padding_y
    omf.close()
    cells = np.ascontiguousarray(field[::2, ::2]).astype(np.int16)
    assert np.array_equal(cells.astype(np.float32).repeat(2, 0).repeat(2, 1), field)
    q4, st = bbme.subpel_cells(p1, p2, cells)
    epe_int = flow.CalculateMSE(gt, cells_to_field(cells, px, py, w, h, 1))
    epe_ref = flow.CalculateMSE(gt, cells_to_field(q4, px, py, w, h, 4))
    u1, u2 = bbme.resize_x4(f1), bbme.resize_x4(f2)
    omf = oracle.OracleMF(u1, u2, [64] * 4, [32] * 4)
    big = omf.calc_motion_block_matching()
    epe_x4 = flow.CalculateMSE(gt, bbme.subsample_div4(big, omf.padding_x, omf.padding_y, w, h))
    omf.close()
    valid = st["valid"] / float(cells.shape[0] * cells.shape[1])
    with capsys.disabled():
        print("\nsubpel quality, Venus pair %dx%d: integer %.4f px, refined %.4f px, x4 pipeline %.4f px; %.1f %% of the cells valid, "
              "%.1f %% of those moved, window SAD %.2f -> %.2f per cell"
              % (w, h, epe_int, epe_ref, epe_x4, 100 * valid, 100.0 * st["moved"] / st["valid"],
                 st["cost_integer"] / st["valid"], st["cost_refined"] / st["valid"]))
    assert valid >= 0.90
    assert epe_ref <= 0.6 * epe_int
    assert epe_ref <= 0.20


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
    assert "SUBPEL RULE" in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    d = buf.ctypes.data
    # a null context is refused before anything touches a device
    assert L.bbme_cells_subpel_device(None, d, d, d, None, d, 8, st, None) == inv
    assert L.bbme_subpel_device(None, 0, 0, d, 8, None) == inv
    assert L.bbme_get_subpel_cells_host(None, 0, 0, d) == inv
    assert L.bbme_subpel_stats(None, 0, None, st) == inv
    assert L.bbme_get_subpel_flow_host(None, 0, 0, d) == inv
    assert hasattr(bbme, "subpel_cells")
    for name in ("subpel_cells", "subpel_flow", "subpel_stats", "cells_subpel_device"):
        assert hasattr(bbme.MF, name), name
    for cls in (bbme.MFBatch, bbme.MFChain):
        for name in ("get_pair_subpel_cells", "get_pair_subpel_flow", "subpel_stats_all"):
            assert hasattr(cls, name), name
    import inspect
    from blockbasedmotionestimation_amd import sequence
    assert "subpel" in inspect.signature(sequence.estimate_frames_pipelined).parameters


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    H, W = 12, 16
    img = np.zeros((H, W), np.uint8)
    g = np.zeros((H // 2, W // 2, 2), np.int16)
    out = np.zeros((H // 2, W // 2, 2), np.int16)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    I, G = img.ctypes.data, g.ctypes.data

    def call(a=I, b=I, w=W, h=H, cells=G, win=None, o=out.ctypes.data, t=st):
        return L.bbme_subpel_host(a, b, w, h, cells, win, o, t)

    assert call() == 0
    assert call(a=None) == inv and call(b=None) == inv and call(cells=None) == inv
    assert call(o=None, t=None) == inv                                            # nothing asked for
    assert call(o=None) == 0 and call(t=None) == 0
    assert call(w=W - 1) == inv and call(h=H - 1) == inv                          # odd sizes
    assert call(w=0) == inv and call(h=0) == inv
    CW, CH = W // 2, H // 2
    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (CW - 1, 0, 2, 2), (0, CH - 1, 2, 2), (0, 0, CW + 1, CH)):
        assert call(win=(C.c_int * 4)(*win)) == inv, win
    assert call(win=(C.c_int * 4)(CW - 2, CH - 2, 2, 2)) == 0
    # beyond 8188 a valid cell's quarter-pel vector need not fit 16 bits: refused before a byte is read
    assert call(w=8190, h=2) == _capi.ERR_UNSUPPORTED and call(w=2, h=8190) == _capi.ERR_UNSUPPORTED
    with pytest.raises(bbme.BbmeError) as e:
        bbme.subpel_cells(img, img, g[:, :4])
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        bbme.subpel_cells(img, img[:, :8], g)
    assert e.value.status == inv
