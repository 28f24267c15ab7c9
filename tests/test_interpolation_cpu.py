"""CPU tests of the interpolation rule (include/bbme.h, "INTERPOLATION RULE"): the C-ABI exports the interpolation calls;
bbme_interpolate_host follows the rule, which is restated here in vectorised numpy from the header's text and imported by the GPU
tests; properties that need no oracle (zero grids, a global translation, ties, every quotient of the blend) carry their answers
written out; on videos of constant motion the interpolated middle frame beats the average of its neighbours."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import INT16_SPECIALS
from test_gpu_bidirectional import CASES, _frames, _oracle_fields

NEW_SYMBOLS = ["bbme_cells_interpolate_device", "bbme_interpolate_device", "bbme_get_interpolated_host", "bbme_interpolation_stats",
               "bbme_interpolate_host"]

STAT_KEYS = ("forward", "backward", "zero", "cost")

# (num, den): den in {2, 3, 4, 5, 255, 256}, the first, a middle and the last phase of the large ones
PHASES = [(1, 2), (1, 3), (2, 3), (1, 4), (3, 4), (2, 5), (4, 5), (1, 255), (128, 255), (254, 255), (1, 256), (77, 256), (255, 256)]
DIVISION_DENS = (2, 3, 5, 7, 16, 24, 25, 30, 60, 255, 256)


def np_interpolate(I1, I2, F, B, num, den, window=None):
    """The rule of include/bbme.h: output cell (cx, cy) with origin o = (2 cx, 2 cy) tries v = F[cy, cx], v = -B[cy, cx] (B may
    be None) and v = 0, in this order; s = floor((num v + den // 2) / den) per component, p1 = o - s, p2 = p1 + v; valid when
    both 2x2 cells lie inside the plane; cost = sum |I1[p1 + (j, i)] - I2[p2 + (j, i)]|; the valid hypothesis of the smallest
    cost wins, the earliest of equals; out = ((den - num) I1[p1 ..] + num I2[p2 ..] + den // 2) // den.  Returns (out uint8
    (H0, W0), sel uint8 (CH, CW), (cells that selected 0, 1, 2, sum of the selected costs) over window (cx0, cy0, cw, ch) in
    cells, None = all cells)."""
    I1 = np.asarray(I1).astype(np.int64)
    I2 = np.asarray(I2).astype(np.int64)
    H0, W0 = I1.shape
    CH, CW = H0 // 2, W0 // 2
    F = np.asarray(F).astype(np.int64)
    hyps = [(0, F)]
    if B is not None:
        hyps.append((1, -np.asarray(B).astype(np.int64)))
    hyps.append((2, np.zeros((CH, CW, 2), np.int64)))
    cy, cx = np.mgrid[0:CH, 0:CW]
    ox, oy = 2 * cx, 2 * cy
    big = 1 << 40
    best = np.full((CH, CW), big, np.int64)
    sel = np.full((CH, CW), 255, np.int64)
    pix = np.zeros((2, 2, CH, CW), np.int64)
    for k, v in hyps:
        vx, vy = v[..., 0], v[..., 1]
        p1x, p1y = ox - (num * vx + den // 2) // den, oy - (num * vy + den // 2) // den          # numpy's // floors
        p2x, p2y = p1x + vx, p1y + vy
        valid = ((p1x >= 0) & (p2x >= 0) & (p1x <= W0 - 2) & (p2x <= W0 - 2) &
                 (p1y >= 0) & (p2y >= 0) & (p1y <= H0 - 2) & (p2y <= H0 - 2))
        q1x, q1y, q2x, q2y = (np.where(valid, p, 0) for p in (p1x, p1y, p2x, p2y))
        cost = np.zeros((CH, CW), np.int64)
        blend = np.zeros((2, 2, CH, CW), np.int64)
        for i in range(2):
            for j in range(2):
                a, b = I1[q1y + i, q1x + j], I2[q2y + i, q2x + j]
                cost += np.abs(a - b)
                blend[i, j] = ((den - num) * a + num * b + den // 2) // den
        take = valid & (cost < best)                       # strictly cheaper: the earliest of equals stays
        best = np.where(take, cost, best)
        sel = np.where(take, k, sel)
        pix = np.where(take[None, None], blend, pix)
    assert (sel != 255).all()                              # k = 2 is always valid
    out = np.empty((H0, W0), np.uint8)
    for i in range(2):
        for j in range(2):
            out[i::2, j::2] = pix[i, j]
    if window is None:
        window = (0, 0, CW, CH)
    x0, y0, w, h = window
    s, c = sel[y0:y0 + h, x0:x0 + w], best[y0:y0 + h, x0:x0 + w]
    return out, sel.astype(np.uint8), (int((s == 0).sum()), int((s == 1).sum()), int((s == 2).sum()), int(c.sum()))


def host_interpolate(bbme, I1, I2, F, B, num, den, window=None):
    out, sel, st = bbme.interpolate_cells(I1, I2, F, B, num, den, window)
    return out, sel, tuple(st[k] for k in STAT_KEYS)


def assert_host_equals_numpy(bbme, I1, I2, F, B, num, den, window, what=None):
    exp = np_interpolate(I1, I2, F, B, num, den, window)
    got = host_interpolate(bbme, I1, I2, F, B, num, den, window)
    tag = (what, num, den, B is not None, window)
    assert np.array_equal(got[0], exp[0]), tag
    assert np.array_equal(got[1], exp[1]), tag
    assert got[2] == exp[2], tag
    return exp


def odd_windows(CH, CW):
    return [None, (1, 1, CW - 3, CH - 2), (CW // 3, CH // 2, 1, 1), (CW - 5, CH - 3, 5, 3), (0, CH // 3, CW, 1)]


def padded_planes(bbme, name):
    """The level-0 padded planes a context holds of CASES[name] (host restatement: x4 up-sampling, zero border)."""
    w, h, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    if up == 4:
        f1, f2 = bbme.resize_x4(f1), bbme.resize_x4(f2)
    _, _, px, py = bbme.plan_padding(w * up, h * up, search, block)
    return bbme.pad_zero(f1, px, py), bbme.pad_zero(f2, px, py)


def oracle_grids(bbme, oracle, name):
    """The oracle's forward and backward 2x2-cell grids of CASES[name] (shared with tests/test_gpu_bidirectional.py's cache)."""
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    _, fwd = _oracle_fields(bbme, oracle, f1, f2, search, block, up, key=(name, "f"))
    _, bwd = _oracle_fields(bbme, oracle, f2, f1, search, block, up, key=(name, "b"))
    return fwd, bwd


def random_grids(CH, CW, rng, reach=5):
    """Small vectors with vectors of up to the plane's size sprinkled in: hypotheses leave the plane on every side."""
    f = rng.integers(-reach, reach + 1, (CH, CW, 2)).astype(np.int16)
    b = rng.integers(-reach, reach + 1, (CH, CW, 2)).astype(np.int16)
    for g in (f, b):
        far = rng.random((CH, CW)) < 0.15
        g[far] = np.stack([rng.integers(-2 * CW, 2 * CW + 1, (CH, CW)), rng.integers(-2 * CH, 2 * CH + 1, (CH, CW))], -1)[far]
    return f, b


def extreme_grids(CH, CW, rng):
    """Every cell one of the int16 extremes: every such hypothesis leaves any plane of fewer than 16 384 pixels a side."""
    specials = np.array(INT16_SPECIALS + [(-32768, 0), (0, 32767), (32767, -32768), (0, -32767)], np.int16)
    return specials[rng.integers(0, len(specials), (CH, CW))], specials[rng.integers(0, len(specials), (CH, CW))]


def ramp_pair():
    """256 x 256 planes I1[y][x] = x, I2[y][x] = y: with zero grids the blend meets every numerator (den - num) a + num b + den / 2."""
    y, x = np.mgrid[0:256, 0:256]
    return x.astype(np.uint8), y.astype(np.uint8)


def ramp_expected(num, den):
    y, x = np.mgrid[0:256, 0:256]
    return (((den - num) * x + num * y + den // 2) // den).astype(np.uint8)              # Python-exact in int64


def _box5(a):
    pad = np.pad(a, 2, mode="edge")
    c = np.cumsum(pad, axis=0, dtype=np.float64)
    c = np.vstack([np.zeros((1, c.shape[1])), c])
    v = c[5:] - c[:-5]
    c = np.cumsum(v, axis=1, dtype=np.float64)
    c = np.hstack([np.zeros((c.shape[0], 1)), c])
    return (c[:, 5:] - c[:, :-5]) / 25.0


def constant_motion_video(w, h, seed, mm, tiles):
    """Three frames of one band-limited texture whose tiles x tiles tiles each move by a constant vector per frame (components
    in -mm // 2 .. mm // 2), frames 1 and 2 with +-2 noise: frame 1 is the true middle of frames 0 and 2."""
    m = 2 * mm
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(h + 2 * m, w + 2 * m)).astype(np.float64)
    for _ in range(3):
        base = _box5(base)
    base -= base.min()
    base *= 255 / base.max()
    base = np.rint(base).astype(np.uint8)
    mv = np.random.default_rng(seed + 1).integers(-mm // 2, mm // 2 + 1, size=(tiles, tiles, 2))
    ty = np.minimum(np.arange(h) * tiles // h, tiles - 1)
    tx = np.minimum(np.arange(w) * tiles // w, tiles - 1)
    mo = mv[ty[:, None], tx[None, :]]                      # (h, w, 2) = (dx, dy) per pixel
    ys, xs = np.mgrid[0:h, 0:w]
    noise = np.random.default_rng(seed + 2)                # draws for frame 1, then frame 2
    frames = []
    for k in (0, 1, 2):
        f = base[ys - k * mo[..., 1] + m, xs - k * mo[..., 0] + m].astype(np.int16)
        if k > 0:
            f = f + noise.integers(-2, 3, size=f.shape)
        frames.append(np.clip(f, 0, 255).astype(np.uint8))
    return frames


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10.0 * np.log10(255.0 ** 2 / np.mean(d * d))


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbme.h")).read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
    assert "INTERPOLATION RULE" in header
    L = _capi.lib()
    buf = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID
    # a null context is refused before anything touches a device
    assert L.bbme_cells_interpolate_device(None, 0, buf.ctypes.data, buf.ctypes.data, 1, 1, 2, None, buf.ctypes.data, 8, 0,
                                           buf.ctypes.data, 4, 0, st, None) == inv
    assert L.bbme_interpolate_device(None, 0, 1, 1, 2, buf.ctypes.data, 8, 0, None) == inv
    assert L.bbme_get_interpolated_host(None, 0, 1, 2, buf.ctypes.data) == inv
    assert L.bbme_interpolation_stats(None, 1, 2, None, st) == inv
    assert hasattr(bbme, "interpolate_cells")
    for name in ("interpolate", "interpolate_run", "interpolation_stats", "cells_interpolate_device"):
        assert hasattr(bbme.MF, name), name
    for name in ("get_pair_interpolated", "interpolation_stats_all"):
        assert hasattr(bbme.MFBatch, name), name
        assert hasattr(bbme.MFChain, name), name
    from blockbasedmotionestimation_amd import sequence
    assert hasattr(sequence, "interpolate_frames")


def test_context_calls_need_a_device(bbme):
    """Without a GPU no context exists to interpolate on: its creation is BBME_ERR_HIP, there is no CPU fallback behind the
    context-level calls (the rule on the CPU is bbme_interpolate_host, asked for by name)."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from blockbasedmotionestimation_amd import _capi
    z = np.zeros((64, 64), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MF(z, z, [32], [16]).interpolate()
    assert e.value.status == _capi.ERR_HIP and "no CPU fallback" in e.value.message


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    H, W = 12, 16
    img = np.zeros((H, W), np.uint8)
    g = np.zeros((H // 2, W // 2, 2), np.int16)
    out = np.zeros((H, W), np.uint8)
    sel = np.zeros((H // 2, W // 2), np.uint8)
    st = (C.c_ulonglong * 4)()
    inv = _capi.ERR_INVALID

    def call(i1=img.ctypes.data, i2=img.ctypes.data, w=W, h=H, f=g.ctypes.data, b=g.ctypes.data, num=1, den=2, win=None,
             o=out.ctypes.data, s=sel.ctypes.data, t=st):
        return L.bbme_interpolate_host(i1, i2, w, h, f, b, num, den, win, o, s, t)

    assert call() == 0
    assert call(b=None) == 0                                # the backward grid is optional
    assert call(i1=None) == inv and call(i2=None) == inv and call(f=None) == inv
    assert call(o=None, s=None, t=None) == inv              # nothing asked for
    assert call(o=None) == 0 and call(s=None) == 0 and call(t=None) == 0 and call(o=None, s=None) == 0
    for den in (1, 0, -2, 257):
        assert call(den=den) == inv, den
    assert call(den=256, num=255) == 0 and call(den=2, num=1) == 0
    for num, den in ((0, 2), (2, 2), (-1, 4), (4, 4), (256, 256), (5, 3)):
        assert call(num=num, den=den) == inv, (num, den)
    assert call(w=W - 1) == inv and call(h=H - 1) == inv    # odd sizes
    assert call(w=0) == inv and call(h=0) == inv
    CW, CH = W // 2, H // 2
    for win in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 2), (0, 0, 2, 0), (CW - 1, 0, 2, 2), (0, CH - 1, 2, 2), (0, 0, CW + 1, CH)):
        assert call(win=(C.c_int * 4)(*win)) == inv, win
    assert call(win=(C.c_int * 4)(CW - 2, CH - 2, 2, 2)) == 0
    with pytest.raises(bbme.BbmeError) as e:
        bbme.interpolate_cells(img, img, g[:, :4])
    assert e.value.status == inv


@pytest.mark.parametrize("name", list(CASES))
def test_host_rule_equals_numpy_on_the_oracles_fields(bbme, oracle, name):
    I1, I2 = padded_planes(bbme, name)
    fwd, bwd = oracle_grids(bbme, oracle, name)
    CH, CW = fwd.shape[:2]
    assert I1.shape == (2 * CH, 2 * CW)
    wins = odd_windows(CH, CW)
    seen = set()
    for n, (num, den) in enumerate(PHASES):
        for B in (bwd, None):
            exp = assert_host_equals_numpy(bbme, I1, I2, fwd, B, num, den, wins[n % len(wins)], name)
            seen |= set(np.unique(exp[1]).tolist())
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("H0,W0", [(48, 64), (52, 76), (34, 60), (80, 12), (38, 134)])        # CW 32, 38, 30, 6 and an odd 67
def test_host_rule_equals_numpy_on_random_grids(bbme, H0, W0):
    rng = np.random.default_rng(1000 * H0 + W0)
    I1 = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    I2 = np.clip(I1.astype(np.int16) + rng.integers(-40, 41, (H0, W0)), 0, 255).astype(np.uint8)      # near enough for k = 0 / 1 to win
    CH, CW = H0 // 2, W0 // 2
    f, b = random_grids(CH, CW, rng)
    wins = odd_windows(CH, CW)
    seen = set()
    for n, (num, den) in enumerate(PHASES):
        for B in (b, None):
            exp = assert_host_equals_numpy(bbme, I1, I2, f, B, num, den, wins[n % len(wins)])
            seen |= set(np.unique(exp[1]).tolist())
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("H0,W0", [(48, 64), (34, 60)])
def test_int16_extremes_leave_only_the_zero_hypothesis(bbme, H0, W0):
    rng = np.random.default_rng(7 * H0 + W0)
    I1 = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    I2 = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    CH, CW = H0 // 2, W0 // 2
    f, b = extreme_grids(CH, CW, rng)
    zero = np.zeros((CH, CW, 2), np.int16)
    for num, den in PHASES:
        for B in (b, None):
            out, sel, st = assert_host_equals_numpy(bbme, I1, I2, f, B, num, den, None)
            assert (sel == 2).all() and st[:3] == (0, 0, CH * CW)
            assert np.array_equal(out, np_interpolate(I1, I2, zero, None, num, den)[0])


def test_zero_grids_blend_in_place(bbme):
    rng = np.random.default_rng(31)
    H0, W0 = 40, 56
    I1 = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    I2 = rng.integers(0, 256, (H0, W0)).astype(np.uint8)
    z = np.zeros((H0 // 2, W0 // 2, 2), np.int16)
    sad = int(np.abs(I1.astype(np.int64) - I2.astype(np.int64)).sum())
    for num, den in PHASES:
        out, sel, st = host_interpolate(bbme, I1, I2, z, z, num, den)
        assert not sel.any()                                # all three hypotheses tie: the first wins
        assert np.array_equal(out, (((den - num) * I1.astype(np.int64) + num * I2.astype(np.int64) + den // 2) // den).astype(np.uint8))
        assert st == (H0 * W0 // 4, 0, 0, sad)
        assert np_interpolate(I1, I2, z, z, num, den)[2] == st


@pytest.mark.parametrize("d", [(6, -4), (-2, 8), (0, 2), (-10, -6)])
def test_global_even_translation_is_followed_half_way(bbme, d):
    dx, dy = d
    H0, W0, m = 64, 96, 16
    rng = np.random.default_rng(41)
    base = rng.integers(0, 256, (H0 + 2 * m, W0 + 2 * m)).astype(np.float64)
    base = np.rint(_box5(base)).astype(np.uint8)
    I1 = base[m:m + H0, m:m + W0]
    I2 = base[m - dy:m - dy + H0, m - dx:m - dx + W0]      # I2[y][x] = I1[y - dy][x - dx]
    mid = base[m - dy // 2:m - dy // 2 + H0, m - dx // 2:m - dx // 2 + W0]
    f = np.empty((H0 // 2, W0 // 2, 2), np.int16)
    f[...] = d
    out, sel, _ = host_interpolate(bbme, I1, I2, f, -f, 1, 2)
    r = max(abs(dx), abs(dy))                               # inside this margin both 2x2 cells stay in the plane
    assert np.array_equal(out[r:H0 - r, r:W0 - r], mid[r:H0 - r, r:W0 - r])
    assert not sel[r // 2 + 1:(H0 - r) // 2 - 1, r // 2 + 1:(W0 - r) // 2 - 1].any()
    exp = np_interpolate(I1, I2, f, -f, 1, 2)
    assert np.array_equal(out, exp[0]) and np.array_equal(sel, exp[1])


def test_ties_go_to_the_earliest_valid_hypothesis(bbme):
    H0, W0 = 24, 32
    flat = np.full((H0, W0), 77, np.uint8)
    CH, CW = H0 // 2, W0 // 2
    rng = np.random.default_rng(5)
    f = rng.integers(-2, 3, (CH, CW, 2)).astype(np.int16)
    f[0], f[-1], f[:, 0], f[:, -1] = 0, 0, 0, 0             # every forward hypothesis stays inside
    b = rng.integers(-1, 2, (CH, CW, 2)).astype(np.int16)
    b[0], b[-1], b[:, 0], b[:, -1] = 0, 0, 0, 0
    out, sel, st = host_interpolate(bbme, flat, flat, f, b, 1, 2)
    assert not sel.any() and (out == 77).all() and st == (CH * CW, 0, 0, 0)
    f[3, 4] = (W0, 0)                                       # points outside the plane: k = 0 is invalid there, k = 1 wins the tie
    f[5, 6] = (0, -H0)
    out, sel, st = host_interpolate(bbme, flat, flat, f, b, 1, 2)
    exp = np.zeros((CH, CW), np.uint8)
    exp[3, 4] = exp[5, 6] = 1
    assert np.array_equal(sel, exp) and st == (CH * CW - 2, 2, 0, 0)
    out, sel, st = host_interpolate(bbme, flat, flat, f, None, 1, 2)      # without B the zero hypothesis is next
    assert np.array_equal(sel, 2 * exp) and st == (CH * CW - 2, 0, 2, 0)
    assert np_interpolate(flat, flat, f, None, 1, 2)[2] == st


@pytest.mark.parametrize("den", DIVISION_DENS)
def test_every_numerator_meets_the_exact_quotient(bbme, den):
    I1, I2 = ramp_pair()
    z = np.zeros((128, 128, 2), np.int16)
    for num in range(1, den):
        out, sel, _ = host_interpolate(bbme, I1, I2, z, None if num % 2 else z, num, den)
        assert np.array_equal(out, ramp_expected(num, den)), num
        assert not sel.any()


# (w, h, search, block, seed, mm, tiles): (cells that selected k = 0, 1, 2 over all cells of the padded plane), from the rule on
# the oracle's two fields (np_interpolate)
QUALITY_CASES = {
    (128, 96, (48, 48), (16, 16), 11, 12, 1): (2413, 521, 138),
    (128, 96, (48, 48), (16, 16), 12, 12, 2): (2111, 528, 433),
    (192, 128, (40, 40), (8, 8), 13, 8, 3): (5208, 610, 326),
    (256, 192, (48, 48), (16, 16), 14, 12, 4): (9327, 2079, 882),
}


@pytest.mark.parametrize("case", list(QUALITY_CASES))
def test_interpolated_middle_frame_beats_the_average(bbme, oracle, case):
    """Estimate (f0, f2) both ways with the oracle and interpolate at 1 / 2: over the interior the PSNR against the true middle
    frame f1 beats the rounded average's by at least 3 dB (a sign or rounding slip in the rule costs far more than that)."""
    w, h, search, block, seed, mm, tiles = case
    search, block = list(search), list(block)
    f0, f1, f2 = constant_motion_video(w, h, seed, mm, tiles)
    _, fwd = _oracle_fields(bbme, oracle, f0, f2, search, block)
    _, bwd = _oracle_fields(bbme, oracle, f2, f0, search, block)
    _, _, px, py = bbme.plan_padding(w, h, search, block)
    I1, I2 = bbme.pad_zero(f0, px, py), bbme.pad_zero(f2, px, py)
    out, sel, st = host_interpolate(bbme, I1, I2, fwd, bwd, 1, 2)
    exp = np_interpolate(I1, I2, fwd, bwd, 1, 2)
    assert np.array_equal(out, exp[0]) and np.array_equal(sel, exp[1]) and st == exp[2]
    mid = out[py:py + h, px:px + w]
    avg = ((f0.astype(np.int32) + f2 + 1) // 2).astype(np.uint8)
    inner = (slice(mm, h - mm), slice(mm, w - mm))
    p_rule, p_avg = psnr(mid[inner], f1[inner]), psnr(avg[inner], f1[inner])
    print("case %s: rule %.1f dB, average %.1f dB, selected %s" % (case, p_rule, p_avg, st[:3]))
    assert p_rule >= p_avg + 3.0, (p_rule, p_avg)
    assert st[0] > 0 and st[1] > 0 and st[2] > 0
    assert st[:3] == QUALITY_CASES[case]
