"""Motion compensation on the GPU (k_motion_compensate: MF::draw_MVimage, motion_framework.cpp:887-905, and its residual
statistics): every frame byte for byte and every statistic exactly what the numpy restatement of include/bbme.h's rule gives
on the oracle's level planes and MVs, after bbme_estimate and in the reference's stage states, and on injected grids (the
counterpart of test_motion_compensation_cpu.test_host_rule_equals_numpy): every block size under every grid block, vectors that
leave on all four sides, that sit exactly at and one past each bound, and int16's extremes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _write_pgm, oracle_schedule
from test_motion_compensation_cpu import block_mvs_from_grid, np_draw_mvimage, np_stats

pytestmark = pytest.mark.gpu

# name: (source width, height, search, block, seed, max motion, upsample)
CASES = {
    "cfg1_like": (200, 136, [30] * 3, [16] * 3, 601, 7, 1),
    "ref2": (376, 250, [32, 32, 42], [16, 16, 32], 602, 10, 1),
    "b8_r32": (160, 96, [72, 72], [8, 8], 603, 24, 1),
    "block2": (160, 128, [12, 20], [2, 4], 604, 4, 1),
    "x4": (48, 36, [30, 30], [16, 16], 605, 3, 4),
    "border_motion": (128, 96, [48, 48], [16, 16], 606, 24, 1),
}


def _frames(bbme, name):
    w, h, _, _, seed, mm, _ = CASES[name]
    f1, f2, _ = bbme.synth_pair(w, h, seed, max_motion=mm)
    if name == "border_motion":
        # one global motion (5, 3): blocks at the right and bottom edges whose MV the larger blocks inherit point outside
        f2 = np.roll(f1, (3, 5), axis=(0, 1))
    return f1, f2


def _blocks(B):
    b = 1
    while b <= B:
        yield b
        b *= 2


def _oracle_after_schedule(bbme, oracle, f1, f2, search, block, upsample):
    if upsample == 4:
        f1, f2 = bbme.resize_x4(f1), bbme.resize_x4(f2)
    omf = oracle.OracleMF(f1, f2, search, block)
    oracle_schedule(omf, len(block))
    return omf


@pytest.mark.parametrize("name", list(CASES))
def test_after_estimate_equals_numpy_on_the_oracle(bbme, oracle, name):
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    mf = bbme.MF(f1, f2, search, block, upsample=up)
    mf.estimate_async()
    omf = _oracle_after_schedule(bbme, oracle, f1, f2, search, block, up)
    assert np.array_equal(mf.get_flow(), omf.flow(0))
    skipped = 0
    unpadded = (mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height)
    for lvl in range(len(block)):
        image1, image2 = omf.image(lvl, 1).copy(), omf.image(lvl, 2).copy()
        a, b_ = mf.get_level_planes(lvl)
        assert np.array_equal(a, image1) and np.array_equal(b_, image2), "planes of level %d" % lvl
        for b in _blocks(block[lvl]):
            mvs = omf.block_mvs(lvl, b)
            for fill in (0, 255):
                exp, ok = np_draw_mvimage(image2, mvs, b, fill)
                got = mf.draw_MVimage(lvl, b, fill)
                assert np.array_equal(got, exp), "level %d block %d fill %d: %d bytes differ" % (lvl, b, fill, (got != exp).sum())
            st = mf.compensation_error(lvl, b, window=(0, 0, image2.shape[1], image2.shape[0]))
            assert (st["sse"], st["sad"], st["pixels"], st["skipped"]) == np_stats(image1, exp, ok), (lvl, b)
            from blockbasedmotionestimation_amd import _capi
            s = (C.c_ulonglong * 4)()
            _capi.check(mf._lib.bbme_compensation_error(mf._ctx, lvl, b, None, s))
            assert tuple(s) == np_stats(image1, exp, ok), (lvl, b)
            if lvl == 0:
                st = mf.compensation_error(0, b)
                assert (st["sse"], st["sad"], st["pixels"], st["skipped"]) == np_stats(image1, exp, ok, unpadded), b
                assert st["mse"] == st["sse"] / st["pixels"]
            skipped += st["skipped"]
    if name == "border_motion":
        assert skipped > 0
    omf.close()
    mf.close()


def test_stage_states_equal_the_oracle(bbme, oracle):
    from blockbasedmotionestimation_amd import _capi
    _, _, search, block, _, _, _ = CASES["border_motion"]
    f1, f2 = _frames(bbme, "border_motion")
    omf = oracle.OracleMF(f1, f2, search, block)
    mf = bbme.MF(f1, f2, search, block)
    levels = len(block)
    for lvl in range(levels):
        mf.set_level_planes(lvl, omf.image(lvl, 1), omf.image(lvl, 2))
    # no grid yet
    with pytest.raises(bbme.BbmeError) as e:
        mf.draw_MVimage(0, 2)
    assert e.value.status == _capi.ERR_STATE
    with pytest.raises(bbme.BbmeError) as e:
        mf.compensation_error(levels - 1, block[-1])
    assert e.value.status == _capi.ERR_STATE

    def check(lvl, bmin, what):
        image1, image2 = omf.image(lvl, 1), omf.image(lvl, 2)
        for b in _blocks(block[lvl]):
            if b < bmin:
                continue
            exp, ok = np_draw_mvimage(image2, omf.block_mvs(lvl, b), b, 0)
            assert np.array_equal(mf.draw_MVimage(lvl, b, 0), exp), "%s: level %d block %d" % (what, lvl, b)
            st = mf.compensation_error(lvl, b, window=(0, 0, image2.shape[1], image2.shape[0]))
            assert (st["sse"], st["sad"], st["pixels"], st["skipped"]) == np_stats(image1, exp, ok), (what, lvl, b)

    for lvl in range(levels - 1, -1, -1):
        B = block[lvl]
        if lvl != levels - 1:
            omf.copy_mvs(lvl)
        omf.calc_level_bm(lvl)
        mf.stage_search(lvl)
        check(lvl, B, "search")                 # "MC_imageL3" (:160-163) on the coarsest level
        b, lam = B, float(B // 2)
        while b > 1:
            for mult in (1, 2):
                omf.set_block_size(lvl, b)
                omf.set_lambda(lvl, lam)
                omf.regularize_mvs(lvl, mult)
                mf.stage_regularize(lvl, b, mult)
            check(lvl, b, "sweeps at %d" % b)
            omf.divide_blocks(lvl)
            b >>= 1
            lam *= 2
        omf.set_block_size(lvl, B)
    omf.set_block_size(0, 2)
    omf.copy_to_all_pixels(0)
    mf.stage_expand()
    assert np.array_equal(mf.get_flow(), omf.flow(0))
    omf.close()
    mf.close()


# name: (width, height, search, block, level the grids are injected at); planes are noise of 0..255, level 1's injected too
INJECT_CONTEXTS = {"b32": (192, 128, [40], [32], 0), "b16_level1": (256, 192, [48, 48], [16, 16], 1)}
INJECT_GRIDS = ("random", "bounds", "extremes")
EXTREMES = [(32767, 32767), (-32767, -32767), (32767, -32767), (-32767, 32767), (-32768, -32768), (32767, 0), (0, -32767)]


@pytest.fixture(scope="module", params=list(INJECT_CONTEXTS))
def inject_context(bbme, request):
    w, h, search, block, level = INJECT_CONTEXTS[request.param]
    rng = np.random.default_rng(w + h)
    mf = bbme.MF(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8), search, block)
    assert (mf.padded_width, mf.padded_height) == (w, h)
    if level:
        mf.set_level_planes(level, rng.integers(0, 256, (h >> level, w >> level), dtype=np.uint8),
                            rng.integers(0, 256, (h >> level, w >> level), dtype=np.uint8))
    image1, image2 = mf.get_level_planes(level)
    assert image2.shape == (h >> level, w >> level)
    yield mf, level, block[level], image1, image2
    mf.close()


def _bound_targets(size, b):
    """Source positions of a b-block along one axis: one before the plane, the first and the last inside, one past the last."""
    return (-1, 0, size - b, size - b + 1)


def _injected_grid(kind, rows, cols, gb, b, W, H, rng):
    """(rows, cols, 2) int16 grid at grid block gb for b-blocks.  random: vectors of up to half the plane, so that blocks leave on
    all four sides.  bounds: grid block number i puts the source of its first b-block at _bound_targets(W)[i % 4] and
    _bound_targets(H)[i // 4 % 4].  extremes: zeros mixed with int16's extremes."""
    if kind == "random":
        return np.stack([rng.integers(-W // 2, W // 2 + 1, (rows, cols)), rng.integers(-H // 2, H // 2 + 1, (rows, cols))], -1).astype(np.int16)
    if kind == "bounds":
        gy, gx = np.mgrid[0:rows, 0:cols]
        i = gy * cols + gx
        tx, ty = np.array(_bound_targets(W, b))[i % 4], np.array(_bound_targets(H, b))[i // 4 % 4]
        return np.stack([tx - gx * gb, ty - gy * gb], -1).astype(np.int16)
    grid = np.zeros((rows, cols, 2), np.int16)
    hit = rng.random((rows, cols)) < 0.5
    hit.flat[:2] = (True, False)
    grid[hit] = np.array(EXTREMES, np.int16)[rng.integers(0, len(EXTREMES), int(hit.sum()))]
    return grid


@pytest.mark.parametrize("kind", INJECT_GRIDS)
def test_injected_grids_equal_numpy(bbme, inject_context, kind):
    from blockbasedmotionestimation_amd import _capi
    mf, level, B, image1, image2 = inject_context
    H, W = image2.shape
    rng = np.random.default_rng(len(kind) + W)
    windows = ((0, 0, W, H), (5, 3, W - 11, H - 8))
    combos, leaves = 0, np.zeros(4, bool)                     # a block left at the left, right, top, bottom
    for b in _blocks(B):
        for gb in sorted({2, b, B}):
            if b > gb:
                continue
            if gb < 2:                                          # a grid is held at 2..B: there is no 1 x 1 grid to inject
                with pytest.raises(bbme.BbmeError) as e:
                    mf.stage_set_mvs(level, gb, np.zeros((H, W, 2), np.int16))
                assert e.value.status == _capi.ERR_INVALID
                continue
            rows, cols = H // gb, W // gb
            grid = _injected_grid(kind, rows, cols, gb, b, W, H, rng)
            mf.stage_set_mvs(level, gb, grid)
            mvs = block_mvs_from_grid(grid.astype(np.int32), gb, b, H, W)
            for fill in (0, 255):
                exp, ok = np_draw_mvimage(image2, mvs, b, fill)
                got = mf.draw_MVimage(level, b, fill)
                assert np.array_equal(got, exp), "block %d under %d, fill %d: %d bytes differ" % (b, gb, fill, (got != exp).sum())
            for window in windows:
                st = mf.compensation_error(level, b, window)
                assert (st["sse"], st["sad"], st["pixels"], st["skipped"]) == np_stats(image1, exp, ok, window), (b, gb, window)
            first = ok[::gb, ::gb]                              # the first b-block of every grid block
            if kind == "random":
                ys, xs = np.mgrid[0:H:b, 0:W:b]
                sx, sy = xs + mvs[..., 0], ys + mvs[..., 1]
                leaves |= np.array([(sx < 0).any(), (sx > W - b).any(), (sy < 0).any(), (sy > H - b).any()])
                assert ok.any() and not ok.all(), (b, gb)
            elif kind == "bounds":
                i = np.arange(rows * cols).reshape(rows, cols)
                assert len(np.unique(i % 16)) == 16
                inside_x, inside_y = np.isin(i % 4, (1, 2)), np.isin(i // 4 % 4, (1, 2))
                assert np.array_equal(first, inside_x & inside_y), (b, gb)
                for other, this in ((inside_y, i % 4), (inside_x, i // 4 % 4)):          # accepted at, rejected one past, every bound
                    for at, past in ((1, 0), (2, 3)):
                        assert first[other & (this == at)].all() and not first[other & (this == past)].any(), (b, gb)
            else:
                moved = (mvs != 0).any(-1)
                zero = np.repeat(np.repeat(~moved, b, 0), b, 1)
                assert moved.any() and not moved.all()
                assert np.array_equal(ok, zero) and np.array_equal(exp, np.where(zero, image2, 255))
                assert mf.compensation_error(level, b, windows[0])["skipped"] == int(moved.sum()) * b * b
            combos += 1
    assert combos == {32: 11, 16: 9}[B] and (kind != "random" or leaves.all())


def test_injected_grid_into_a_strided_view(bbme, inject_context):
    import torch
    mf, level, B, _, image2 = inject_context
    H, W = image2.shape
    grid = _injected_grid("random", H // B, W // B, B, 4, W, H, np.random.default_rng(W))
    mf.stage_set_mvs(level, B, grid)
    for b in (1, 4, B):
        exp, _ = np_draw_mvimage(image2, block_mvs_from_grid(grid.astype(np.int32), B, b, H, W), b, 9)
        big = torch.full((H, W + 13), 0xAB, dtype=torch.uint8, device="cuda")
        mf.motion_compensated_device(big[:, :W], level, b, 9)
        mf.synchronize()
        got = big.cpu().numpy()
        assert np.array_equal(got[:, :W], exp) and (got[:, W:] == 0xAB).all(), b


def test_batch_equals_single_contexts(bbme):
    search, block = [30, 30, 30], [16, 16, 16]
    pairs = [bbme.synth_pair(200, 136, 700 + i, max_motion=6 + 4 * i)[:2] for i in range(3)]
    mb = bbme.MFBatch(pairs, search, block)
    mb.estimate_async()
    singles = []
    for p in pairs:
        mf = bbme.MF(p[0], p[1], search, block)
        mf.estimate_async()
        singles.append(mf)
    for lvl, b in ((0, 2), (0, 1), (1, 8), (2, 16)):
        got = mb.compensation_errors(lvl, b)
        assert len(got) == 3
        for i, mf in enumerate(singles):
            assert got[i] == mf.compensation_error(lvl, b), (lvl, b, i)
            assert np.array_equal(mb.get_pair_motion_compensated(i, lvl, b, 9), mf.draw_MVimage(lvl, b, 9)), (lvl, b, i)
    assert mb.compensation_error() == singles[0].compensation_error()
    assert len({r["sse"] for r in mb.compensation_errors()}) == 3
    for mf in singles:
        mf.close()
    mb.close()


def test_device_output_into_a_strided_view_on_a_side_stream(bbme):
    import torch
    f1, f2, _ = bbme.synth_pair(200, 136, 801, max_motion=7)
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3)
    mf.estimate_async()
    s = torch.cuda.Stream()
    for lvl, b, fill in ((0, 2, 0), (0, 1, 255), (1, 16, 3), (2, 4, 0)):
        W, H, _, _ = mf.level_geometry(lvl)
        exp = mf.draw_MVimage(lvl, b, fill)
        for extra in (13, 16):                                  # rows not 4-byte aligned, and aligned
            big = torch.full((H, W + extra), 0xAB, dtype=torch.uint8, device="cuda")
            mf.motion_compensated_device(big[:, :W], lvl, b, fill, s.cuda_stream)
            s.synchronize()
            got = big.cpu().numpy()
            assert np.array_equal(got[:, :W], exp), (lvl, b, extra)
            assert (got[:, W:] == 0xAB).all(), (lvl, b, extra)
    big = torch.full((mf.padded_height, mf.padded_width), 0xAB, dtype=torch.uint8, device="cuda")
    mf.motion_compensated_device(big)
    mf.synchronize()
    assert np.array_equal(big.cpu().numpy(), mf.draw_MVimage())
    mf.close()


def test_errors_and_no_state_change(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    f1, f2, _ = bbme.synth_pair(200, 136, 901, max_motion=7)
    search, block = [30] * 3, [16] * 3
    mf = bbme.MF(f1, f2, search, block)
    flow = mf.calcMotionBlockMatching()
    cells = mf.get_cells()
    W, H, _, _ = mf.level_geometry(0)
    W2, H2, _, _ = mf.level_geometry(2)
    out = np.zeros((H, W), np.uint8)
    st = (C.c_ulonglong * 4)()
    dev = mf.flow_device_ptr()
    ctx = mf._ctx
    inv = _capi.ERR_INVALID
    for pair, lvl, b, fill in ((1, 0, 2, 0), (-1, 0, 2, 0), (0, 3, 2, 0), (0, -1, 2, 0), (0, 0, 3, 0), (0, 0, 0, 0),
                               (0, 0, 32, 0), (0, 0, 2, -1), (0, 0, 2, 256)):
        assert L.bbme_get_motion_compensated_host(ctx, pair, lvl, b, fill, out.ctypes.data) == inv, (pair, lvl, b, fill)
        assert L.bbme_motion_compensate_device(ctx, pair, lvl, b, fill, C.c_void_p(dev), W, None) == inv, (pair, lvl, b, fill)
    for lvl, b in ((3, 2), (-1, 2), (0, 3), (0, 0), (0, 32), (2, 32)):
        assert L.bbme_compensation_error(ctx, lvl, b, None, st) == inv, (lvl, b)
    assert L.bbme_get_motion_compensated_host(ctx, 0, 0, 2, 0, None) == inv
    assert L.bbme_motion_compensate_device(ctx, 0, 0, 2, 0, None, W, None) == inv
    assert L.bbme_motion_compensate_device(ctx, 0, 0, 2, 0, C.c_void_p(dev), W - 1, None) == inv
    assert L.bbme_compensation_error(ctx, 0, 2, None, None) == inv
    for win in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (W - 7, 0, 8, 8), (0, H - 7, 8, 8),
                (0, 0, W + 1, H)):
        assert L.bbme_compensation_error(ctx, 0, 2, (C.c_int * 4)(*win), st) == inv, win
    assert L.bbme_compensation_error(ctx, 2, 2, (C.c_int * 4)(0, 0, W2, H2 + 1), st) == inv
    assert L.bbme_compensation_error(ctx, 2, 2, (C.c_int * 4)(0, 0, W2, H2), st) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.draw_MVimage(0, 2, out=np.zeros((H, W + 1), np.uint8))
    assert e.value.status == inv
    # a run of valid calls leaves the context as it was
    for lvl in range(3):
        for b in _blocks(block[lvl]):
            mf.draw_MVimage(lvl, b)
            mf.compensation_error(lvl, b)
    assert np.array_equal(mf.get_flow(), flow)
    assert np.array_equal(mf.get_cells(), cells)
    # the other getters' scratch buffers (grown here) and the compensation's are independent
    mc, err = mf.draw_MVimage(), mf.compensation_error()
    mf.get_subsampled_flow(4)
    mf.get_subsampled_flow(1)
    assert np.array_equal(mf.draw_MVimage(), mc) and mf.compensation_error() == err
    assert np.array_equal(mf.calcMotionBlockMatching(), flow)
    mf.close()


def test_cli_writes_the_compensated_frame(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    f1, f2, _ = bbme.synth_pair(96, 72, 1001, max_motion=3)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    args = ["--levels", "3", "--block", "16", "--search", "30"]
    base = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm")] + args
    r0 = subprocess.run(base + ["--out", str(tmp_path / "a.flo"), "--color", str(tmp_path / "a.ppm")], capture_output=True,
                        text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    r1 = subprocess.run(base + ["--out", str(tmp_path / "b.flo"), "--color", str(tmp_path / "b.ppm"), "--mc",
                                str(tmp_path / "mc.pgm")], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert (tmp_path / "a.flo").read_bytes() == (tmp_path / "b.flo").read_bytes()
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    assert "MC PSNR" not in r0.stdout
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3, upsample=4)
    mf.estimate_async()
    mc = mf.draw_MVimage(0, 2, 0)
    px, py, w, h = mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height
    assert (tmp_path / "mc.pgm").read_bytes() == b"P5\n%d %d\n255\n" % (w, h) + mc[py:py + h, px:px + w].tobytes()
    e = mf.compensation_error()
    assert "MC PSNR is %.9g dB over %d pixels (%d skipped)\n" % (e["psnr"], e["pixels"], e["skipped"]) in r1.stdout
    assert e["pixels"] + e["skipped"] == w * h
    mf.close()
