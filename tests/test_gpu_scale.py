"""The gather kernels where the benchmark runs them and the other tests do not: planes of 2 Mpixel, the smallest at which every
statistics kernel leaves more than 256 partials per pair, so that lanes of k_mc_reduce take a second trip, the last workgroup of a
launch is partly filled, every cell row ends inside a lane's run and both paddings are odd (tests/test_scale_cpu.py recomputes all
of that from the kernels' constants and proves the content non-trivial).  Injected planes and grids on single contexts; every pair
of a batch and every frame of a chain from one launch, on fields read back from the context, so that nothing here depends on what
the estimate found.  Global motion and global compensation (K16, K17, K18, K18b) on injected grids and planes at that shape and at
the rule's widest and tallest plane, 8188 (section d; tests/test_global_motion_scale_cpu.py is its CPU side).  Every comparison is
exact, against the numpy restatements of include/bbme.h's rules in tests/test_*_cpu.py."""
import numpy as np
import pytest

import helpers as H
from test_bgr_cpu import np_interpolate_bgr
from test_consistency_cpu import STAT_KEYS as FB_KEYS, leaving_grids, np_cells_consistency
from test_global_compensation_bgr_cpu import np_global_compensate_bgr
from test_global_motion_cpu import COMP_MODELS, MODELS, np_global_compensate, np_histogram, np_moments
from test_gpu_bgr import _device_bgr
from test_gpu_bidirectional import _device_consistency
from test_gpu_global_compensation_bgr import _warp
from test_gpu_global_motion import _compensate, _hist, _moments
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


# ---- d. global motion and global compensation at G1 and at the rule's widest and tallest plane ----------------------------------
def _bare_context(bbme, g, name):
    z = np.zeros((g["h"], g["w"]), np.uint8)
    mf = bbme.MF(z, z, g["search"], g["block"])                    # frames set, no estimate: the device calls need neither
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == H.GM_PADDED[name] + (1, 1)
    return mf


@pytest.fixture(scope="module")
def gm_wide(bbme):
    mf = _bare_context(bbme, H.GM_WIDE, "WIDE")
    yield mf
    mf.close()


@pytest.fixture(scope="module")
def gm_tall(bbme):
    mf = _bare_context(bbme, H.GM_TALL, "TALL")
    yield mf
    mf.close()


@pytest.fixture
def gm_context(request):
    """(name, context) of SCALE_G1, GM_WIDE or GM_TALL"""
    if request.param == "G1":
        return "G1", request.getfixturevalue("g1")["mf"]
    return request.param, request.getfixturevalue({"WIDE": "gm_wide", "TALL": "gm_tall"}[request.param])


GM_NAMES = ("G1", "WIDE", "TALL")


@pytest.mark.parametrize("gm_context", GM_NAMES, indirect=True)
def test_vector_histogram_strides_over_the_runs(gm_context):
    """K16 where its 256 workgroups take a second and a third trip through the runs and the last trip ends inside a workgroup"""
    name, mf = gm_context
    CH, CW = mf.cells_shape
    grids, mask = H.gm_histogram_grids(CH, CW)
    window = H.gm_cell_window(CW, CH)
    for gname, g in grids:
        exp = np_histogram(g)
        assert np.array_equal(_hist(mf, g), exp), (name, gname)
        if gname == "uniform":
            assert exp.max() == CH * CW > 2 ** 17
        got = _hist(mf, g, mask, window, q_extra=5, e_extra=3, twice=True)            # twice: the call zeroes the table
        assert np.array_equal(got, np_histogram(g, mask, window)), (name, gname, "mask and window")


@pytest.mark.parametrize("gm_context", GM_NAMES, indirect=True)
def test_global_moments_sum_beyond_32_bits_over_more_than_16_workgroups(gm_context):
    """K17 where words 6..8 pass 2^40 and words 11..14 pass 2^31 (GM_WIDE, GM_TALL) and k_reduce_words<16> takes up to nine
    trips with an uneven last one"""
    import torch
    name, mf = gm_context
    CH, CW = mf.cells_shape
    g, true, mask = H.gm_scale_grid(CH, CW)
    window = H.gm_cell_window(CW, CH)
    side = torch.cuda.Stream()
    for k, (model, tol) in enumerate(((true, H.GM_TOL), (MODELS[3], 2 ** 40), (MODELS[4], 2 ** 40))):
        exp = np_moments(g, model, tol, mask, window)
        got = _moments(mf, g, model, tol, mask, window, map_offset=1 + k, map_extra=2, q_extra=k, e_extra=3,
                       stream=side if k == 1 else None)
        assert np.array_equal(got[0], exp[0]), (name, model, np.argwhere(got[0] != exp[0])[:4])
        assert np.array_equal(got[1], exp[1]), (name, model, got[1], exp[1])
        assert exp[1][0] > 0 and exp[1][1] > 0 and exp[1][2] > 0
    exp = np_moments(g, true, H.GM_TOL)
    got = _moments(mf, g, true, H.GM_TOL, want=("words",))
    assert got[0] is None and np.array_equal(got[1], exp[1]), (name, "words alone", got[1], exp[1])
    got = _moments(mf, g, true, H.GM_TOL, want=("map",), map_offset=3, map_extra=8)
    assert got[1] is None and np.array_equal(got[0], exp[0]), (name, "map alone")


@pytest.mark.parametrize("gm_context", GM_NAMES, indirect=True)
def test_global_compensation_sums_beyond_32_bits_over_more_than_256_workgroups(gm_context):
    """K18 where its partials take k_mc_reduce's lanes into a second trip and sse passes 2^32"""
    name, mf = gm_context
    W0, H0 = mf.padded_width, mf.padded_height
    I1, I2 = H.gm_scale_planes(H0, W0)
    odd = H.gm_plane_window(W0, H0)
    beyond = 0
    for k, (model, unit) in enumerate(COMP_MODELS[:4]):
        fill, win = (0, 7, 255)[k % 3], (None, odd)[k % 2]
        exp = np_global_compensate(I1, I2, model, unit, fill, win)
        frame, st = _compensate(mf, I1, I2, model, unit, fill, win, out_offset=1 + k % 3, out_extra=(3, 0, 8)[k % 3])
        assert np.array_equal(frame, exp[0]), (name, model, unit, np.argwhere(frame != exp[0])[:4])
        assert st == exp[1], (name, model, unit, win, st, exp[1])
        beyond += exp[1][0] > 2 ** 32
        if k == 2:
            assert min(exp[1][2], exp[1][3]) >= (win[2] * win[3] if win else W0 * H0) // 4           # compensates and skips in bulk
        if k == 1:                                             # the statistics alone over the other window, the frame alone
            other = np_global_compensate(I1, I2, model, unit, fill, None)
            assert _compensate(mf, I1, I2, model, unit, fill, None, want=("stats",)) == (None, other[1])
            frame, st = _compensate(mf, None, I2, model, unit, fill, want=("out",), out_offset=5)
            assert st is None and np.array_equal(frame, other[0])
    assert beyond >= 3
    for unit, (tx, ty) in ((1, (3, -2)), (4, (-5, 7))):            # the whole-pixel property
        frame, _ = _compensate(mf, None, I2, (tx * unit << 16, 0, 0, ty * unit << 16, 0, 0), unit, 77, want=("out",))
        exp = np.full((H0, W0), 77, np.uint8)
        exp[max(0, -ty):H0 - max(0, ty), max(0, -tx):W0 - max(0, tx)] = I2[max(0, ty):H0 - max(0, -ty), max(0, tx):W0 - max(0, -tx)]
        assert np.array_equal(frame, exp), (name, unit, tx, ty)
    # the largest sums: every pixel differs by 255
    _, st = _compensate(mf, np.zeros_like(I1), np.full_like(I1, 255), (0,) * 6, 1, want=("stats",))
    assert st == (255 * 255 * W0 * H0, 255 * W0 * H0, W0 * H0, 0) and st[0] > 2 ** 32


@pytest.mark.parametrize("gm_context", GM_NAMES[:2], indirect=True)
def test_colour_global_compensation_of_three_frames_from_one_launch(gm_context):
    """K18b on colour frames of 2058 x 1038 and 8186 x 130: three frames under three models from one launch, 523 and 260 partials
    per frame"""
    name, mf = gm_context
    h, w = mf.orig_height, mf.orig_width
    c1, c2, models, unit, window = H.gm_scale_bgr_case(h, w)
    got, st = _warp(mf, c1, c2, models, unit, 3, window, in_extra=1, out_extra=5, out_offset=1)
    for k in range(3):
        exp = np_global_compensate_bgr(c1[k], c2[k], models[k], unit, 3, mf.padding_x, mf.padding_y, window)
        assert np.array_equal(got[k], exp[0]), (name, k, np.argwhere(got[k] != exp[0])[:4])
        assert st[k] == exp[1], (name, k, st[k], exp[1])
        assert exp[1][0] > 2 ** 32
    assert H.stats_differ_pairwise(st, words=(0, 1)), st
