"""The gather kernels where the benchmark runs them and the other tests do not: planes of 2 Mpixel, the smallest at which every
statistics kernel leaves more than 256 partials per pair, so that lanes of k_mc_reduce take a second trip, the last workgroup of a
launch is partly filled, every cell row ends inside a lane's run and both paddings are odd (tests/test_scale_cpu.py recomputes all
of that from the kernels' constants and proves the content non-trivial).  Injected planes and grids on single contexts; every pair
of a batch and every frame of a chain from one launch, on fields read back from the context, so that nothing here depends on what
the estimate found.  Every comparison is exact, against the numpy restatements of include/bbme.h's rules in tests/test_*_cpu.py."""
import numpy as np
import pytest

import helpers as H
from test_bgr_cpu import np_interpolate_bgr
from test_consistency_cpu import STAT_KEYS as FB_KEYS, leaving_grids, np_cells_consistency
from test_gpu_bgr import _device_bgr
from test_gpu_bidirectional import _device_consistency
from test_gpu_interpolation import _device_interpolate
from test_gpu_temporal_filter import _device_filter
from test_interpolation_cpu import STAT_KEYS as IP_KEYS, np_interpolate
from test_motion_compensation_cpu import block_mvs_from_grid, np_draw_mvimage, np_stats
from test_temporal_filter_cpu import STAT_KEYS as TF_KEYS, np_temporal_filter

pytestmark = pytest.mark.gpu

MC_KEYS = ("sse", "sad", "pixels", "skipped")


def _tuples(dicts, keys):
    return [tuple(d[k] for k in keys) for d in dicts]


def _geometry(mf, g):
    """The padded size the shape was chosen for, and its (default, odd) cell windows."""
    assert (mf.padding_x, mf.padding_y) == (1, 1) and mf.padded_width == 2060
    assert mf.padded_height == {1038: 1040, 2070: 2072}[g["h"]]
    default, odd = H.scale_cell_windows(mf.padding_x, mf.padding_y, g["w"], g["h"])
    assert default == tuple(mf.default_cell_window())
    return default, odd


# ---- a. injected planes and grids on one context at G1 ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def g1(bbme):
    g = H.SCALE_G1
    f1, f2 = H.scale_frames(g["h"], g["w"], 2)
    mf = bbme.MF(f1, f2, g["search"], g["block"])
    default, odd = _geometry(mf, g)
    I1, I2 = mf.get_level_planes(0)
    assert np.array_equal(I1, bbme.pad_zero(f1, 1, 1)) and np.array_equal(I2, bbme.pad_zero(f2, 1, 1))
    yield dict(mf=mf, I1=I1, I2=I2, odd=odd, grids=H.scale_grids(*mf.cells_shape))
    mf.close()


def test_temporal_filter_on_injected_planes(g1):
    mf, odd = g1["mf"], g1["odd"]
    cur, prev, gp, nxt, gn = H.scale_filter_content(mf.padded_height, mf.padded_width)
    thr = H.SCALE_STRENGTH
    for window in (None, odd):
        exp = np_temporal_filter(cur, prev, gp, nxt, gn, thr, window)
        out, wmap, st = _device_filter(mf, cur, prev, gp, nxt, gn, thr, window, pitch_extra=3)
        assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1]), window
        assert st == exp[2], (window, st, exp[2])
    _, _, st = _device_filter(mf, cur, prev, gp, nxt, gn, thr, odd, want=("stats",))
    assert st == exp[2], ("statistics only", st, exp[2])
    for P, GP, N, GN, what in ((prev, gp, None, None, "previous only"), (None, None, nxt, gn, "next only")):
        exp = np_temporal_filter(cur, P, GP, N, GN, 1021)
        out, wmap, st = _device_filter(mf, cur, P, GP, N, GN, 1021)
        assert np.array_equal(out, exp[0]) and np.array_equal(wmap, exp[1]), what
        assert st == exp[2], (what, st, exp[2])


def test_interpolation_phases_and_a_scratch_buffer_that_grows(g1):
    mf, I1, I2, odd = g1["mf"], g1["I1"], g1["I2"], g1["odd"]
    f, b = g1["grids"]
    expected = {}

    def check(num0, count, den, what):
        out, sel, st = _device_interpolate(mf, f, b, num0, count, den, odd, pitch_extra=2)
        for q in range(count):
            key = (num0 + q, den)
            if key not in expected:
                expected[key] = np_interpolate(I1, I2, f, b, num0 + q, den, odd)
            exp = expected[key]
            assert np.array_equal(out[q], exp[0]) and np.array_equal(sel[q], exp[1]), (what, key)
            assert st[q] == exp[2], (what, key, st[q], exp[2])
        return st

    st = check(1, 3, 4, "three phases from one launch")
    assert H.stats_differ_pairwise(st), st
    check(1, 1, 4, "one phase, in the scratch of three")
    check(1, 5, 6, "five phases: the scratch buffer is replaced")


def test_colour_interpolation(g1):
    mf, I1, I2 = g1["mf"], g1["I1"], g1["I2"]
    f, b = g1["grids"]
    g = H.SCALE_G1
    c1, c2 = H.scale_bgr_frames(g["h"], g["w"])
    got = _device_bgr(mf, f, b, 1, 2, 3, colour=(c1, c2), out_extra=1)
    for q in range(2):
        assert np.array_equal(got[q], np_interpolate_bgr(I1, I2, c1, c2, f, b, 1 + q, 3, mf.padding_x, mf.padding_y)), q


def test_compensation_on_an_injected_grid(bbme):
    g = H.SCALE_G1
    B = g["block"][0]
    f1, f2, grid = H.scale_mc_content(g["h"], g["w"], 1040, 2060, B)
    mf = bbme.MF(f1, f2, g["search"], g["block"])
    _geometry(mf, g)
    I1, I2 = mf.get_level_planes(0)
    mf.stage_set_mvs(0, B, grid)
    H0, W0 = I2.shape
    unpadded = (1, 1, g["w"], g["h"])
    for b in (1, 2, 4):
        exp, ok = np_draw_mvimage(I2, block_mvs_from_grid(grid.astype(np.int32), B, b, H0, W0), b, 255)
        for window, np_window in ((None, unpadded), ((0, 0, W0, H0), None), (H.SCALE_MC_WINDOW, H.SCALE_MC_WINDOW)):
            st = mf.compensation_error(0, b, window)
            want = np_stats(I1, exp, ok, np_window)
            assert tuple(st[k] for k in MC_KEYS) == want, (b, window, st, want)
        assert want[0] > 2 ** 32 and want[3] > 0
        if b != 2:
            assert np.array_equal(mf.draw_MVimage(0, b, 255), exp), b
    mf.close()


# ---- b. consistency on one context at G2 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g2(bbme):
    g = H.SCALE_G2
    z = np.zeros((g["h"], g["w"]), np.uint8)
    mf = bbme.MF(z, z, g["search"], g["block"])                    # no estimate: the device call needs none
    _, odd = _geometry(mf, g)
    yield mf, odd
    mf.close()


def test_consistency_of_injected_grids(bbme, g2):
    mf, odd = g2
    CH, CW = mf.cells_shape
    a, b = H.scale_grids(CH, CW)
    for tol in (0, 1):
        for window in (None, odd):
            exp_mask, exp = np_cells_consistency(a, b, tol, window)
            mask, st = _device_consistency(bbme, mf, a, b, tol, window, extra=1)
            assert np.array_equal(mask[:, :CW], exp_mask) and (mask[:, CW:] == 0xAB).all(), (tol, window)
            assert st == exp, (tol, window, st, exp)
    a, b = leaving_grids(CH, CW, np.random.default_rng(H.SCALE_SEED))
    exp_mask, exp = np_cells_consistency(a, b, 1, odd)
    mask, st = _device_consistency(bbme, mf, a, b, 1, odd, extra=1)
    assert np.array_equal(mask[:, :CW], exp_mask) and st == exp, ("leaving", st, exp)
    assert exp[1] > 0 and exp[2] > exp[1]                         # most targets leave the plane


# ---- c. every pair of a batch and every frame of a chain from one launch ----------------------------------------------------
def _batch(bbme, g):
    video = H.scale_video(g["h"], g["w"], 4)
    mb = bbme.MFBatch([(video[0], video[1]), (video[2], video[3])], g["search"], g["block"])
    default, odd = _geometry(mb, g)
    mb.estimate_bidirectional_async()
    fwd = [mb.get_pair_cells(p) for p in range(2)]
    bwd = [mb.get_pair_backward_cells(p) for p in range(2)]
    assert not np.array_equal(fwd[0], fwd[1]) and not np.array_equal(bwd[0], bwd[1])
    return dict(mb=mb, fwd=fwd, bwd=bwd, windows=((None, default), (odd, odd)))


@pytest.fixture(scope="module")
def batch1(bbme):
    ctx = _batch(bbme, H.SCALE_G1)
    mb = ctx["mb"]
    ctx["planes"] = [[mb.frame_plane_tensor(p, which).cpu().numpy() for which in (0, 1)] for p in range(2)]
    yield ctx
    mb.close()


@pytest.fixture(scope="module")
def batch2(bbme):
    ctx = _batch(bbme, H.SCALE_G2)
    yield ctx
    ctx["mb"].close()


def test_batch_compensation_errors(batch1):
    mb, fwd, planes = batch1["mb"], batch1["fwd"], batch1["planes"]
    H0, W0 = planes[0][0].shape
    g = H.SCALE_G1
    for b in (1, 2, 4):
        frames = [np_draw_mvimage(planes[p][1], block_mvs_from_grid(fwd[p].astype(np.int32), 2, b, H0, W0), b, 0) for p in range(2)]
        for window, np_window in ((None, (1, 1, g["w"], g["h"])), (H.SCALE_MC_WINDOW, H.SCALE_MC_WINDOW)):
            want = [np_stats(planes[p][0], frames[p][0], frames[p][1], np_window) for p in range(2)]
            got = _tuples(mb.compensation_errors(0, b, window), MC_KEYS)
            assert got == want, (b, window, got, want)
            assert H.stats_differ_pairwise(want, words=(0, 1)), want      # (pixels + skipped is the window's size in every pair)


def _check_batch_consistency(ctx):
    mb, fwd, bwd = ctx["mb"], ctx["fwd"], ctx["bwd"]
    for which, A, B in (("forward", fwd, bwd), ("backward", bwd, fwd)):
        for window, np_window in ctx["windows"]:
            want = [np_cells_consistency(A[p], B[p], 1, np_window)[1] for p in range(2)]
            got = _tuples(mb.consistency_stats_all(which, 1, window), FB_KEYS)
            assert got == want, (which, window, got, want)
            assert H.stats_differ_pairwise(want, absent_ok=True), want            # (the estimate never points outside)


def test_batch_consistency_stats(batch1):
    _check_batch_consistency(batch1)


def test_batch_consistency_stats_at_262_workgroups(batch2):
    _check_batch_consistency(batch2)


def test_batch_interpolation_stats(batch1):
    mb, fwd, bwd, planes = batch1["mb"], batch1["fwd"], batch1["bwd"], batch1["planes"]
    for window, np_window in batch1["windows"]:
        want = [np_interpolate(planes[p][0], planes[p][1], fwd[p], bwd[p], 1, 2, np_window)[2] for p in range(2)]
        got = _tuples(mb.interpolation_stats_all(1, 2, window), IP_KEYS)
        assert got == want, (window, got, want)
        assert H.stats_differ_pairwise(want), want


def test_batch_temporal_filter_stats(batch1):
    mb, fwd, bwd, planes = batch1["mb"], batch1["fwd"], batch1["bwd"], batch1["planes"]
    thr = H.SCALE_STRENGTH
    for window, np_window in batch1["windows"]:
        want = []
        for p in range(2):
            want.append(np_temporal_filter(planes[p][0], None, None, planes[p][1], fwd[p], thr, np_window)[2])
            want.append(np_temporal_filter(planes[p][1], planes[p][0], bwd[p], None, None, thr, np_window)[2])
        got = _tuples(mb.temporal_filter_stats(thr, window), TF_KEYS)
        assert got == want, (window, got, want)
        assert H.stats_differ_pairwise(want, absent_ok=True), want


@pytest.fixture(scope="module")
def chain1(bbme):
    g = H.SCALE_G1
    video = H.scale_video(g["h"], g["w"], 3)
    chain = bbme.MFChain(video, g["search"], g["block"])
    default, _ = _geometry(chain, g)
    chain.estimate_bidirectional_async()
    ctx = dict(chain=chain, default=default, planes=[chain.get_slot_plane(0, s) for s in range(3)],
               fwd=[chain.get_pair_cells(p) for p in range(2)], bwd=[chain.get_pair_backward_cells(p) for p in range(2)])
    assert not np.array_equal(ctx["fwd"][0], ctx["fwd"][1])
    yield ctx
    chain.close()


def test_chain_temporal_filter_of_every_slot(chain1):
    chain, planes, fwd, bwd = chain1["chain"], chain1["planes"], chain1["fwd"], chain1["bwd"]
    thr = H.SCALE_STRENGTH
    want = [np_temporal_filter(planes[s], planes[s - 1] if s > 0 else None, bwd[s - 1] if s > 0 else None,
                               planes[s + 1] if s < 2 else None, fwd[s] if s < 2 else None, thr, chain1["default"]) for s in range(3)]
    stats = [w[2] for w in want]
    got = _tuples(chain.temporal_filter_stats(thr), TF_KEYS)
    assert got == stats, (got, stats)
    assert H.stats_differ_pairwise(stats, absent_ok=True), stats
    assert stats[0][0] == 0 and stats[2][1] == 0 and min(stats[1][:2]) > 0       # the first has no previous, the last no next
    run = chain.temporal_filter_run(thr)
    for s in range(3):
        assert np.array_equal(run[s], want[s][0]), s
