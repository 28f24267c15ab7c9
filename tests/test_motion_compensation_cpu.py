"""CPU tests of motion compensation (MF::draw_MVimage, motion_framework.cpp:887-905, and its residual statistics): the C-ABI
exports it, bbme_motion_compensate_host follows the rule of include/bbme.h, which is restated here in numpy from the
reference's text, and a finished level's 2x2 grid is all the rule needs to reproduce the oracle's draw_MVimage."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import oracle_schedule

NEW_SYMBOLS = ["bbme_motion_compensate_device", "bbme_get_motion_compensated_host", "bbme_compensation_error",
               "bbme_motion_compensate_host", "bbme_pgm_write"]


def np_draw_mvimage(image2, mvs, b, fill):
    """draw_MVimage (:887-905): block (X, Y) = (bx b, by b) with MV mvs[by, bx] = (dx, dy) copies the b x b block of
    image2 at (X + dx, Y + dy) unless that leaves the plane (:899); skipped pixels get `fill`.
    Returns (frame, mask of compensated pixels)."""
    H, W = image2.shape
    ys, xs = np.mgrid[0:H, 0:W]
    by, bx = ys // b, xs // b
    sx = bx * b + mvs[by, bx, 0]
    sy = by * b + mvs[by, bx, 1]
    ok = (sx >= 0) & (sx <= W - b) & (sy >= 0) & (sy <= H - b)
    src_y = np.where(ok, sy + ys - by * b, 0)
    src_x = np.where(ok, sx + xs - bx * b, 0)
    return np.where(ok, image2[src_y, src_x], fill).astype(np.uint8), ok


def np_stats(image1, frame, ok, window=None):
    """(sse, sad, pixels, skipped) over window (x0, y0, w, h); skipped pixels are in neither sum."""
    if window is not None:
        x0, y0, w, h = window
        image1, frame, ok = image1[y0:y0 + h, x0:x0 + w], frame[y0:y0 + h, x0:x0 + w], ok[y0:y0 + h, x0:x0 + w]
    d = frame.astype(np.int64) - image1.astype(np.int64)
    return (int((d[ok] ** 2).sum()), int(np.abs(d[ok]).sum()), int(ok.sum()), int((~ok).sum()))


def block_mvs_from_grid(grid, grid_block, b, H, W):
    """MVs at the origins of the b-blocks: the grid entry covering pixel (X, Y) (include/bbme.h)."""
    oy = np.arange(0, H, b) // grid_block
    ox = np.arange(0, W, b) // grid_block
    return grid[oy[:, None], ox[None, :]]


def host_mc(image1, image2, grid, grid_block, b, fill, window=None, frame=True, stats=True):
    from blockbasedmotionestimation_amd import _capi
    H, W = image2.shape
    grid = np.ascontiguousarray(grid, np.int16)
    out = np.full((H, W), 0x5A, np.uint8) if frame else None
    st = (C.c_ulonglong * 4)() if stats else None
    win = None if window is None else (C.c_int * 4)(*window)
    rc = _capi.lib().bbme_motion_compensate_host(image1.ctypes.data if image1 is not None else None, image2.ctypes.data, W, H,
                                                 grid.ctypes.data, grid_block, b, fill, win,
                                                 out.ctypes.data if frame else None, st)
    assert rc == 0, _capi.lib().bbme_last_error()
    return out, (tuple(st) if stats else None)


def test_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    L = _capi.lib()
    out = np.zeros(64, np.uint8)
    st = (C.c_ulonglong * 4)()
    # a null context is refused before anything touches a device
    assert L.bbme_motion_compensate_device(None, 0, 0, 2, 0, out.ctypes.data, 8, None) == _capi.ERR_INVALID
    assert L.bbme_get_motion_compensated_host(None, 0, 0, 2, 0, out.ctypes.data) == _capi.ERR_INVALID
    assert L.bbme_compensation_error(None, 0, 2, None, st) == _capi.ERR_INVALID


@pytest.mark.parametrize("W,H", [(64, 48), (70, 54), (38, 26), (96, 34)])
def test_host_rule_equals_numpy(bbme, W, H):
    rng = np.random.default_rng(W * 1000 + H)
    image1 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    image2 = rng.integers(0, 256, (H, W), dtype=np.uint8)
    B = 32
    skipped = compensated = 0
    for b in (1, 2, 4, 8, 16, 32):
        for gb in sorted({2, b, B}):
            # MVs large enough to leave the plane on all four sides
            grid = rng.integers(-W // 2, W // 2 + 1, (-(-H // gb), -(-W // gb), 2)).astype(np.int16)
            grid[..., 1] = rng.integers(-H // 2, H // 2 + 1, grid.shape[:2])
            mvs = block_mvs_from_grid(grid.astype(np.int32), gb, b, H, W)
            for fill in (0, 77, 255):
                exp, ok = np_draw_mvimage(image2, mvs, b, fill)
                got, st = host_mc(image1, image2, grid, gb, b, fill)
                assert np.array_equal(got, exp), (b, gb, fill)
                assert st == np_stats(image1, exp, ok), (b, gb, fill)
            window = (W // 5, H // 4, W // 2, H // 3)
            _, st = host_mc(image1, image2, grid, gb, b, 0, window=window, frame=False)
            assert st == np_stats(image1, exp, ok, window), (b, gb)
            # no statistics without image1; the frame alone is unchanged
            got, _ = host_mc(None, image2, grid, gb, b, 255, stats=False)
            assert np.array_equal(got, exp)
            skipped += int((~ok).sum())
            compensated += int(ok.sum())
    assert skipped > 0 and compensated > 0


def test_host_rule_refuses_bad_arguments(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    z = np.zeros((8, 8), np.uint8)
    g = np.zeros((4, 4, 2), np.int16)
    out = np.zeros((8, 8), np.uint8)
    st = (C.c_ulonglong * 4)()

    def call(img1=z.ctypes.data, img2=z.ctypes.data, w=8, h=8, grid=g.ctypes.data, gb=2, b=2, fill=0, win=None,
             o=out.ctypes.data, s=st):
        return L.bbme_motion_compensate_host(img1, img2, w, h, grid, gb, b, fill, win, o, s)

    assert call() == 0
    assert call(img2=None) == _capi.ERR_INVALID
    assert call(grid=None) == _capi.ERR_INVALID
    assert call(img1=None) == _capi.ERR_INVALID              # statistics need image1
    assert call(img1=None, s=None) == 0
    assert call(o=None, s=None) == _capi.ERR_INVALID         # nothing asked for
    assert call(b=3) == _capi.ERR_INVALID
    assert call(b=0) == _capi.ERR_INVALID
    assert call(fill=-1) == _capi.ERR_INVALID
    assert call(fill=256) == _capi.ERR_INVALID
    assert call(win=(C.c_int * 4)(4, 0, 5, 8)) == _capi.ERR_INVALID
    assert call(win=(C.c_int * 4)(0, 0, 0, 8)) == _capi.ERR_INVALID
    assert call(win=(C.c_int * 4)(4, 4, 4, 4)) == 0


def test_finished_level_needs_only_its_2x2_grid(bbme, oracle):
    """For every level after the whole schedule and every b <= B_l, the oracle's draw_MVimage from block_mvs(l, b) equals
    the rule fed only the level's final 2x2 grid."""
    f1, f2, _ = bbme.synth_pair(168, 120, 515, max_motion=10)
    search, block = [30, 30, 30], [16, 16, 16]
    omf = oracle.OracleMF(f1, f2, search, block)
    oracle_schedule(omf, 3)
    for lvl in range(3):
        image1, image2 = omf.image(lvl, 1).copy(), omf.image(lvl, 2).copy()
        H, W = image2.shape
        grid2 = omf.block_mvs(lvl, 2)
        b = 1
        while b <= block[lvl]:
            for fill in (0, 255):
                exp, ok = np_draw_mvimage(image2, omf.block_mvs(lvl, b), b, fill)
                got, st = host_mc(image1, image2, grid2, 2, b, fill)
                assert np.array_equal(got, exp), (lvl, b, fill)
                assert st == np_stats(image1, exp, ok), (lvl, b, fill)
            b *= 2
    omf.close()


def test_pgm_write_and_cli_usage(bbme, tmp_path):
    from blockbasedmotionestimation_amd import _capi, build as _build
    L = _capi.lib()
    W, H, pitch = 7, 5, 12
    buf = np.arange(H * pitch, dtype=np.uint8).reshape(H, pitch)
    path = tmp_path / "a.pgm"
    assert L.bbme_pgm_write(str(path).encode(), W, H, pitch, buf.ctypes.data) == 0
    assert path.read_bytes() == b"P5\n%d %d\n255\n" % (W, H) + buf[:, :W].tobytes()
    assert L.bbme_pgm_write(str(path).encode(), W, H, W - 1, buf.ctypes.data) == _capi.ERR_INVALID
    assert L.bbme_pgm_write(str(tmp_path / "no" / "a.pgm").encode(), W, H, pitch, buf.ctypes.data) == _capi.ERR_IO
    r = subprocess.run([_build.CLI], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: bbme_cli" in r.stderr and "--mc" in r.stderr
