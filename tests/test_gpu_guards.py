"""What a result comparison cannot see: writes outside a kernel's buffers, and reads of words nothing has written.

Every context here is created under BBME_TEST_GUARD=1 and BBME_TEST_POISON=1 (include/bbme.h, "test hooks"): every device
allocation of the library lies between two guard bands of 4096 bytes, and every data buffer that is not zeroed or uploaded starts
as 0xC7 in every byte (DESIGN.md section 4 has the table of who writes and reads each buffer first).  Each test runs its calls,
compares the results bit for bit with the oracle or the host rule -- the comparisons of the other GPU modules, imported from them --
and then asks bbme_test_guard_check for the guards: no damaged band, and at least as many live guarded buffers as a context of that
many levels allocates (a knob that silently did nothing fails there).  After the context is closed the check runs again: a buffer
that was freed or replaced had its guards scanned at that moment, and damage found then is remembered.

MIN_LIVE: a context allocates 7 work buffers (flow, list[0..1], flags[0..1], own, counters) and per level 10 (img1, small[0..1],
big[0..1], pred, fix_list, fix_count, publish, spiral); a level the strip kernel serves (blocks of 8 / 16 / 32, range <= 63) has 7
more (rank_of and, per plan, tasks, rounds, lane_ranks).  The SAD memo, the upload buffer and the scratch of the single entry points
come on top."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from test_gpu_context_state import GEOMETRIES as STATE_GEOMETRIES, _pair as _content_pair

pytestmark = pytest.mark.gpu

GUARD = 4096


def min_live(search, block, contexts=1):
    fast = sum(1 for s, b in zip(search, block) if b in (8, 16, 32) and max(s - b, 0) // 2 <= 63)
    return contexts * (7 + 10 * len(block) + 7 * fast)


class Guards:
    """The three test hooks, and the state of the registry when the test began (contexts of other tests are unguarded)."""

    def __init__(self):
        from blockbasedmotionestimation_amd import _capi
        self.capi, self.lib = _capi, _capi.lib()
        self.contexts = []
        _capi.check(self.lib.bbme_test_guard_reset())
        self.base_live, violations, first = self.check()
        assert violations == 0, first

    def own(self, mf):
        """A context of this test: closed when the test ends, however it ends (a failed test must not leave guarded buffers to the next)."""
        self.contexts.append(mf)
        return mf

    def check(self):
        live, violations = C.c_ulonglong(), C.c_ulonglong()
        first = C.create_string_buffer(512)
        self.capi.check(self.lib.bbme_test_guard_check(C.byref(live), C.byref(violations), first, len(first)))
        return live.value, violations.value, first.value.decode()

    def clean(self, at_least, what=""):
        """No damaged guard, and at least `at_least` guarded buffers of this test's contexts alive."""
        live, violations, first = self.check()
        assert violations == 0, "%s: %d damaged guard bands, the first: %s" % (what, violations, first)
        assert live - self.base_live >= at_least, "%s: %d guarded buffers alive, a context allocates at least %d" % (
            what, live - self.base_live, at_least)
        return live - self.base_live

    def closed(self, what=""):
        """Every context of the test is closed: the freed buffers' record is clean and nothing of the test is alive."""
        live, violations, first = self.check()
        assert violations == 0, "%s, after close: %d damaged guard bands, the first: %s" % (what, violations, first)
        assert live == self.base_live, "%s: %d guarded buffers still alive after close" % (what, live - self.base_live)


@pytest.fixture
def guards(monkeypatch):
    """Both knobs for the whole test: the scratch of the single entry points is allocated on first use, not at creation."""
    monkeypatch.setenv("BBME_TEST_GUARD", "1")
    monkeypatch.setenv("BBME_TEST_POISON", "1")
    g = Guards()
    yield g
    for mf in g.contexts:
        mf.close()


def _same_field(got, exp, what):
    bad = np.argwhere((got != exp).any(-1))
    assert bad.size == 0, "%s: %d of %d pixels differ, first at %s: reference %s gpu %s" % (
        what, len(bad), exp.shape[0] * exp.shape[1], bad[0], exp[tuple(bad[0])], got[tuple(bad[0])])


# ---- the estimate path ----------------------------------------------------------------------------------------------------------
# name: (width, height, search, block, how the frames are made) -- the smallest geometries at which each edge exists
ESTIMATE_GEOMETRIES = {
    "padded_both_ways": (250, 130, [30], [16], ("synth", 1015, 5)),
    "b2_alone": (128, 96, [10], [2], ("synth", 1028, 3)),
    "b2_between": (192, 128, [14, 10, 24], [4, 2, 8], ("synth", 1030, 5)),
    "two_block_rows": (1024, 64, [48, 48], [16, 16], ("synth", 1016, 12)),
    "two_block_columns": (64, 1024, [48, 48], [16, 16], ("synth", 1017, 12)),
    "r63_lane_ranks_slack": (384, 256, [134], [8], ("synth", 1022, 60)),
    "r64_generic_large_window": (384, 256, [144], [16], ("synth", 1025, 60)),
    "b64": (512, 512, [80, 80], [64, 64], ("synth", 1012, 10)),
    "odd_shift": (256, 128, [17, 21], [16, 16], ("synth", 1009, 3)),
    "state_fast": STATE_GEOMETRIES["fast"] + (("content", 1, 4101),),
    "state_generic": STATE_GEOMETRIES["generic"] + (("content", 4, 4102),),
}
SCHEDULES = {
    "default": {},
    "speculate_all_late": {"BBME_SPEC_MIN_GABS": "0", "BBME_SPEC_LATE": "2"},
    "no_graph": {"BBME_NO_GRAPH": "1"},
    "stagewise": None,
}
_REFERENCE = {}


def _estimate_reference(bbme, oracle, name):
    """(f1, f2, the oracle's planes per level, its stage grids, its field) of a geometry, computed once and left unchanged."""
    if name not in _REFERENCE:
        w, h, search, block, (kind, a, b) = ESTIMATE_GEOMETRIES[name]
        if kind == "synth":
            f1, f2, _ = bbme.synth_pair(w, h, a, max_motion=b)
        else:
            f1, f2 = _content_pair(a, w, h, np.random.default_rng(b))
        omf = oracle.OracleMF(f1, f2, search, block)
        planes = [(omf.image(l, 1).copy(), omf.image(l, 2).copy()) for l in range(len(block))]
        stages = []
        flow = H.oracle_schedule(omf, len(block), lambda *s: stages.append(s))
        omf.close()
        flow.setflags(write=False)
        _REFERENCE[name] = (f1, f2, planes, stages, flow)
    return _REFERENCE[name]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("name", list(ESTIMATE_GEOMETRIES))
def test_estimate_between_guards(bbme, oracle, monkeypatch, guards, name, schedule):
    w, h, search, block, _ = ESTIMATE_GEOMETRIES[name]
    f1, f2, planes, stages, flow = _estimate_reference(bbme, oracle, name)
    what = "%s, %s" % (name, schedule)
    for k, v in (SCHEDULES[schedule] or {}).items():
        monkeypatch.setenv(k, v)
    mf = guards.own(bbme.MF(f1, f2, search, block, len(block)))
    if schedule == "stagewise":
        # the oracle's planes, as compare_stagewise hands them over; every stage's grid against the oracle's
        for lvl, (p1, p2) in enumerate(planes):
            mf.set_level_planes(lvl, p1, p2)
        got = []
        gflow = H.gpu_schedule(mf, len(block), block, lambda *s: got.append(s))
        H.assert_stages_equal(stages, got, what)
        _same_field(gflow, flow, what)
    else:
        for run in ("first", "second"):                      # the second one replays the graph on grids the first one left
            _same_field(mf.calcMotionBlockMatching(), flow, "%s, %s estimate" % (what, run))
    guards.clean(min_live(search, block), what)
    mf.close()
    guards.closed(what)


# ---- forced forms, on content whose windows leave the plane on every side --------------------------------------------------------
FORCED_CONTENTS = ("dark_b16_r16", "border_b16_r32")
FORCED_FORMS = dict({k: (H.LIMIT_REG_FORMS[k], False) for k in ("pass1_strip", "pass1_lanes_low", "solve_one_wave", "relax_rule",
                                                                "memo_b8_forward")},
                    search_split=(H._SPLIT_ON, False), loose_plan=({"BBME_LOOSE_PLAN": "1"}, False),
                    generic_search=({"BBME_GENERIC_SEARCH": "1"}, False), raster=({}, True))
_FORCED = {}


def _forced_reference(oracle, name, raster):
    if (name, raster) not in _FORCED:
        c = H.LIMIT_CONTENTS[name]
        p1, p2 = H.limit_content_planes(name)
        _FORCED[name, raster] = (p1, p2, H.oracle_stages_from_planes(oracle, p1, p2, c["search"], c["block"], raster))
    return _FORCED[name, raster]


@pytest.mark.parametrize("form", list(FORCED_FORMS))
@pytest.mark.parametrize("name", FORCED_CONTENTS)
def test_forced_forms_between_guards(bbme, oracle, monkeypatch, guards, name, form):
    c = H.LIMIT_CONTENTS[name]
    env, raster = FORCED_FORMS[form]
    p1, p2, (stages, flow, _) = _forced_reference(oracle, name, raster)
    what = "%s, %s" % (name, form)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mf = guards.own(H.make_mf_from_planes(bbme, p1, p2, c["search"], c["block"], raster))
    got = []
    gflow = H.gpu_schedule(mf, len(c["block"]), c["block"], lambda *s: got.append(s))
    H.assert_stages_equal(stages, got, what)
    assert np.array_equal(gflow, flow), what
    assert np.array_equal(mf.calcMotionBlockMatching(), flow), what + ", whole estimate"
    guards.clean(min_live(c["search"], c["block"]), what)
    mf.close()
    guards.closed(what)


# ---- other contexts ----------------------------------------------------------------------------------------------------------------
def _oracle_flow(oracle, f1, f2, search, block):
    omf = oracle.OracleMF(f1, f2, search, block)
    flow = omf.calc_motion_block_matching().copy()
    cells = omf.block_mvs(0, 2).astype(np.int16)
    omf.close()
    return flow, cells


def test_batch_of_three_pairs_between_guards(bbme, oracle, guards):
    w, h, search, block = 328, 200, [40] * 3, [8] * 3
    pairs = [bbme.synth_pair(w, h, 5200 + p, max_motion=6 + 2 * p)[:2] for p in range(3)]
    exp = [_oracle_flow(oracle, a, b, search, block)[0] for a, b in pairs]
    mb = guards.own(bbme.MFBatch(pairs, search, block))
    for run in ("first", "second"):
        got = mb.calcMotionBlockMatching()
        for p in range(3):
            _same_field(got[p], exp[p], "pair %d, %s estimate" % (p, run))
    guards.clean(min_live(search, block), "batch")
    mb.close()
    guards.closed("batch")


def test_chain_with_an_advance_between_guards(bbme, oracle, guards):
    w, h, search, block = 200, 120, [30, 30], [16, 16]          # padded in both dimensions (224 x 128)
    frames = bbme.synth_video(w, h, 7, 5300, max_motion=6)
    exp = [_oracle_flow(oracle, frames[k], frames[k + 1], search, block) for k in range(6)]
    chain = guards.own(bbme.MFChain(frames[:4], search, block))
    chain.calcMotionBlockMatching()
    for p in range(3):
        _same_field(chain.get_pair_flow(p), exp[p][0], "pair %d" % p)
        assert np.array_equal(chain.get_pair_cells(p), exp[p][1]), p
    chain.advance(frames[4:7])                              # slot 3 becomes slot 0, three new frames: pairs 3, 4, 5 of the video
    chain.calcMotionBlockMatching()
    for p in range(3):
        _same_field(chain.get_pair_flow(p), exp[p + 3][0], "pair %d behind the advance" % p)
        assert np.array_equal(chain.get_pair_cells(p), exp[p + 3][1]), p
    guards.clean(min_live(search, block), "chain")
    chain.close()
    guards.closed("chain")


def test_bidirectional_between_guards(bbme, oracle, guards):
    from test_gpu_bidirectional import CASES, _both_oracles, _frames
    name = "cfg1_like"
    _, _, search, block, _, _, _ = CASES[name]
    f1, f2 = _frames(bbme, name)
    (fflow, fcells), (_, bcells) = _both_oracles(bbme, oracle, name)
    mf = guards.own(bbme.MF(f1, f2, search, block))
    for run in ("first", "second"):
        mf.estimate_bidirectional_async()
        assert np.array_equal(mf.get_cells(), fcells), run
        assert np.array_equal(mf.get_backward_cells(), bcells), run
        _same_field(mf.get_flow(), fflow, "bidirectional, %s" % run)
    guards.clean(min_live(search, block) + 1, "bidirectional")      # + the backward cells
    mf.close()
    guards.closed("bidirectional")


def test_upsampled_context_between_guards(bbme, oracle, guards):
    w, h, search, block = 48, 40, [30, 30], [16, 16]
    f1, f2, _ = bbme.synth_pair(w, h, 5400, max_motion=2)
    exp, cells = _oracle_flow(oracle, bbme.resize_x4(f1), bbme.resize_x4(f2), search, block)
    mf = guards.own(bbme.MF(f1, f2, search, block, upsample=4))
    _same_field(mf.calcMotionBlockMatching(), exp, "upsample=4")
    sub = mf.get_subsampled_flow()
    from test_flow_color_cpu import subsampled_field
    assert np.array_equal(sub, subsampled_field(cells, mf.orig_width, mf.orig_height, mf.padding_x, mf.padding_y, 4))
    guards.clean(min_live(search, block) + 1, "upsample=4")         # + the upload buffer
    mf.close()
    guards.closed("upsample=4")


# ---- gather stages and getters ---------------------------------------------------------------------------------------------------
# odd paddings (62 -> 64, 46 -> 48, as test_gpu_subpel asserts); 70 cell columns, neither a multiple of 4 nor of a tile
GATHER_GEOMETRIES = [(62, 46, [24, 24], [8, 8]), (140, 98, [12], [2])]
THR = 64


def _gather_context(bbme, oracle, guards, w, h, search, block):
    """A context on two colour frames (the planes are their luma) behind a bidirectional estimate that equals the oracle's."""
    from test_bgr_cpu import np_bgr_to_gray
    from test_temporal_filter_bgr_cpu import near_colour_triple
    c1, _, c2 = near_colour_triple(w, h, 7 * w + h)
    mf = guards.own(bbme.MF(c1, c2, search, block))
    mf.estimate_bidirectional_async()
    g1, g2 = np_bgr_to_gray(c1), np_bgr_to_gray(c2)
    fflow, fcells = _oracle_flow(oracle, g1, g2, search, block)
    _, bcells = _oracle_flow(oracle, g2, g1, search, block)
    assert np.array_equal(mf.get_cells(), fcells) and np.array_equal(mf.get_backward_cells(), bcells)
    _same_field(mf.get_flow(), fflow, "gather context")
    return mf, c1, c2, fcells, bcells


@pytest.mark.parametrize("w,h,search,block", GATHER_GEOMETRIES)
def test_gather_stages_between_guards(bbme, oracle, guards, w, h, search, block):
    import torch
    import test_gpu_bgr as T_bgr
    import test_gpu_flow_color as T_color
    import test_gpu_interpolation as T_ip
    import test_gpu_subpel as T_sp
    import test_gpu_temporal_filter as T_tf
    import test_gpu_temporal_filter_bgr as T_tfc
    from test_bgr_cpu import np_interpolate_bgr
    from test_consistency_cpu import np_cells_consistency
    from test_gpu_bidirectional import _device_consistency
    from test_motion_compensation_cpu import np_draw_mvimage, np_stats
    mf, c1, c2, fwd, bwd = _gather_context(bbme, oracle, guards, w, h, search, block)
    W0, H0, px, py = mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y
    CH, CW = mf.cells_shape
    if w == 62:
        assert px % 2 == 1 and py % 2 == 1
    else:
        assert (W0, H0) == (w, h) and CW == 70 and CW % 4 != 0
    I1, I2 = mf.get_level_planes(0)
    odd = H._odd_window(mf)
    rng = np.random.default_rng(w)
    from test_interpolation_cpu import random_grids
    rf, rb = random_grids(CH, CW, rng)                      # vectors that leave the plane on every side

    # compensation at every level (all of them at 2 x 2 cells behind an estimate): the whole plane and an odd window, a device
    # output one byte wider than packed
    for lvl in range(len(block)):
        lw, lh, _, _ = mf.level_geometry(lvl)
        p1, p2 = mf.get_level_planes(lvl)
        exp, ok = np_draw_mvimage(p2, mf.stage_get_mvs(lvl, 2).astype(np.int32), 2, 7)
        out = torch.full((lh, lw + 1), 0xAA, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        mf.motion_compensated_device(out[:, :lw], lvl, 2, 7)
        mf.synchronize()
        host = out.cpu().numpy()
        assert np.array_equal(host[:, :lw], exp) and (host[:, lw:] == 0xAA).all(), lvl
        for win in ((0, 0, lw, lh), (3, 1, lw - 8, lh - 5)):
            st = mf.compensation_error(lvl, 2, window=win)
            assert (st["sse"], st["sad"], st["pixels"], st["skipped"]) == np_stats(p1, exp, ok, win), (lvl, win)

    # consistency: mask and statistics, each alone, whole and odd window, a mask one byte wider than packed
    for win in (None, odd):
        exp_mask, exp_st = np_cells_consistency(fwd, bwd, 1, win)
        got, st = _device_consistency(bbme, mf, fwd, bwd, 1, win, extra=1)
        assert np.array_equal(got[:, :CW], exp_mask) and (got[:, CW:] == 0xAB).all() and st == exp_st, win
        got, st = _device_consistency(bbme, mf, rf, rb, 1, win, stats=False, extra=1)
        assert np.array_equal(got[:, :CW], np_cells_consistency(rf, rb, 1, win)[0]) and st is None
        got, st = _device_consistency(bbme, mf, rf, rb, 0, win, mask=False)
        assert got is None and st == np_cells_consistency(rf, rb, 0, win)[1]

    # interpolation: three phases in one call
    for win in (None, odd):
        T_ip._assert_device_equals_numpy(mf, I1, I2, fwd, bwd, 1, 3, 4, win, "own fields", pitch_extra=1)
        T_ip._assert_device_equals_numpy(mf, I1, I2, rf, rb, 1, 3, 4, win, "statistics alone", want=("stats",))
    T_ip._assert_device_equals_numpy(mf, I1, I2, rf, None, 1, 3, 4, None, "frames alone", want=("out",), pitch_extra=1)

    # colour interpolation from the stored colour and from a caller's, output rows one byte further apart than packed
    for colour in (None, (c1, c2)):
        got = T_bgr._device_bgr(mf, fwd, bwd, 1, 3, 4, colour, 1 if colour else 0, 1)
        for q in range(3):
            assert np.array_equal(got[q], np_interpolate_bgr(I1, I2, c1, c2, fwd, bwd, 1 + q, 4, px, py)), (colour is None, q)
    got = T_bgr._device_bgr(mf, rf, None, 1, 1, 2, None, 0, 0)
    assert np.array_equal(got[0], np_interpolate_bgr(I1, I2, c1, c2, rf, None, 1, 2, px, py))

    # colour coding with the range found and with a given one, image and range each alone
    for scale in (1, 3):
        T_color._assert_device_equals_host(bbme, mf, rf, scale, -1.0, "range found", pitch_extra=1, offset=1)
        T_color._assert_device_equals_host(bbme, mf, rf, scale, 7.5, "range given, image alone", want=("out",), pitch_extra=1)
        T_color._assert_device_equals_host(bbme, mf, fwd, scale, -1.0, "range alone", want=("range",))

    # temporal filter, grey and colour
    for win in (None, odd):
        T_tf._assert_device_equals_numpy(mf, I1, I2, bwd, I2, fwd, THR, win, "grey", pitch_extra=1)
        T_tf._assert_device_equals_numpy(mf, I1, None, None, I2, rf, THR, win, "grey, statistics alone", want=("stats",))
        T_tfc._assert_device_equals_numpy(mf, c1, c2, bwd, c2, fwd, THR, win, "colour", colour_extra=1, out_extra=1)
        T_tfc._assert_device_equals_numpy(mf, c1, None, None, c2, rf, THR, win, "colour, statistics alone", want=("stats",))
    T_tf._assert_device_equals_numpy(mf, I1, I2, rb, None, None, 255, None, "grey, frame alone", want=("out",), pitch_extra=1)
    T_tfc._assert_device_equals_numpy(mf, c1, c2, rb, None, None, 255, None, "colour, frame alone", want=("out",), out_extra=1)

    # subpel
    for win in (None, odd):
        T_sp._assert_device_equals_host(bbme, mf, I1, I2, fwd, win, "own field", pitch_extra=1)
        T_sp._assert_device_equals_host(bbme, mf, I1, I2, rf, win, "statistics alone", want=("stats",))
    T_sp._assert_device_equals_host(bbme, mf, I2, I1, bwd, None, "grid alone", want=("out",), pitch_extra=1)

    # the device EPE on a ground truth smaller than the frame (the comparison of test_gpu_limits: the header's rel = 1e-12 for
    # another order of the float64 sum)
    gh, gw = h // 2 - 1, w // 2 - 3
    gt = H.epe_ground_truth(gh, gw, "holes", np.random.default_rng(gh))
    assert mf.calculate_mse_device(torch.from_numpy(gt).cuda(), scale=2) == pytest.approx(H.epe_reference(gt, fwd, px, py, 2), rel=1e-12)

    guards.clean(min_live(search, block) + 8, "gather stages")     # + upload buffer or colour store, backward cells, statistics
    mf.close()
    guards.closed("gather stages")


@pytest.mark.parametrize("w,h,search,block", GATHER_GEOMETRIES)
def test_host_getters_grow_the_staging_area_between_guards(bbme, oracle, guards, w, h, search, block):
    """Every host getter in ascending size of its product, so that the staging area is replaced under guard at every step, then
    in descending size inside the area as it is; every product against its rule."""
    from test_bgr_cpu import np_interpolate_bgr
    from test_consistency_cpu import np_cells_consistency
    from test_flow_color_cpu import subsampled_field
    from test_interpolation_cpu import np_interpolate
    from test_motion_compensation_cpu import np_draw_mvimage
    from test_subpel_cpu import cells_to_field
    from test_temporal_filter_bgr_cpu import np_temporal_filter_bgr
    from test_temporal_filter_cpu import np_temporal_filter
    mf, c1, c2, fwd, bwd = _gather_context(bbme, oracle, guards, w, h, search, block)
    px, py = mf.padding_x, mf.padding_y
    I1, I2 = mf.get_level_planes(0)
    top = len(block) - 1
    q4, _ = bbme.subpel_cells(I1, I2, fwd)
    getters = [
        ("consistency", lambda: mf.consistency("forward", 1), lambda: np_cells_consistency(fwd, bwd, 1)[0]),
        ("draw_MVimage, coarsest level", lambda: mf.draw_MVimage(top, 2, 9),
         lambda: np_draw_mvimage(mf.get_level_planes(top)[1], mf.stage_get_mvs(top, 2).astype(np.int32), 2, 9)[0]),
        ("cells", lambda: mf.get_cells(), lambda: fwd),
        ("backward cells", lambda: mf.get_backward_cells(), lambda: bwd),
        ("subpel cells", lambda: mf.subpel_cells("forward"), lambda: q4),
        ("flow colour, scale 2", lambda: mf.flow_color(2), lambda: bbme.color_cells(fwd, w, h, px, py, 2, -1.0)[0]),
        ("draw_MVimage", lambda: mf.draw_MVimage(0, 2, 0), lambda: np_draw_mvimage(I2, fwd.astype(np.int32), 2, 0)[0]),
        ("interpolated", lambda: mf.interpolate(1, 2), lambda: np_interpolate(I1, I2, fwd, bwd, 1, 2)[0]),
        ("temporal filter", lambda: mf.temporal_filter(THR, 0), lambda: np_temporal_filter(I1, None, None, I2, fwd, THR)[0]),
        ("flow colour", lambda: mf.flow_color(1), lambda: bbme.color_cells(fwd, w, h, px, py, 1, -1.0)[0]),
        ("interpolated colour", lambda: mf.interpolate_bgr(1, 2),
         lambda: np_interpolate_bgr(I1, I2, c1, c2, fwd, bwd, 1, 2, px, py)),
        ("temporal filter, colour", lambda: mf.temporal_filter_bgr(THR, 1),
         lambda: np_temporal_filter_bgr(c2, c1, bwd, None, None, THR, px, py)[0]),
        ("interpolated run of 3", lambda: mf.interpolate_run(4),
         lambda: np.stack([np_interpolate(I1, I2, fwd, bwd, n, 4)[0] for n in (1, 2, 3)])),
        ("subsampled flow", lambda: mf.get_subsampled_flow(1), lambda: subsampled_field(fwd, w, h, px, py, 1)),
        ("subpel flow", lambda: mf.subpel_flow("forward"), lambda: cells_to_field(q4, px, py, w, h, 4)),
        ("flow", lambda: mf.get_flow(), lambda: np.repeat(np.repeat(fwd, 2, 0), 2, 1).astype(np.float32)),
    ]
    expected = [(what, rule()) for what, _, rule in getters]
    ascending = sorted(range(len(getters)), key=lambda k: expected[k][1].nbytes)
    assert expected[ascending[0]][1].nbytes < expected[ascending[-1]][1].nbytes
    for order in (ascending, ascending[::-1]):
        for k in order:
            got = getters[k][1]()
            assert got.shape == expected[k][1].shape and np.array_equal(got, expected[k][1]), getters[k][0]
    guards.clean(min_live(search, block) + 3, "host getters")      # + colour store, backward cells, staging area
    mf.close()
    guards.closed("host getters")


# ---- the detector must be able to fail ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back", [1, 0], ids=["back", "front"])
def test_one_damaged_guard_byte_is_reported(bbme, guards, back):
    """One byte of a guard band of the flow field ("work buffers" is the text of the context's first work buffer) overwritten by
    a host-to-device copy -- inside the library's own allocation, so nothing can fault -- is reported with buffer, side and offset."""
    from test_gpu_context_state import _hip
    hip = _hip()
    f1, f2, _ = bbme.synth_pair(128, 96, 1, max_motion=2)
    mf = guards.own(bbme.MF(f1, f2, [20, 20], [8, 8]))
    guards.clean(min_live([20, 20], [8, 8]), "before the damage")
    band = C.c_void_p()
    guards.capi.check(guards.lib.bbme_test_guard_find(b"work buffers", back, C.byref(band)))
    assert band.value and band.value % GUARD == 0
    # offset 5 from the payload's edge: byte 5 of the back band, byte 4095 - 5 of the front band
    at = band.value + (5 if back else GUARD - 1 - 5)
    old, new = (C.c_ubyte * 1)(), (C.c_ubyte * 1)(0x3C)
    assert hip.hipMemcpy(C.addressof(old), at, 1, 2) == 0 and old[0] == 0xA5             # 2: device to host
    assert hip.hipMemcpy(at, C.addressof(new), 1, 1) == 0                                # 1: host to device
    live, violations, first = guards.check()
    assert violations == 1, (violations, first)
    assert first.startswith("work buffers") and ("%s guard, offset 5 from" % ("back" if back else "front")) in first, first
    assert "holds 0x3c" in first and "(1 damaged bytes" in first, first
    assert hip.hipMemcpy(at, C.addressof(old), 1, 1) == 0
    guards.capi.check(guards.lib.bbme_test_guard_reset())
    guards.clean(min_live([20, 20], [8, 8]), "after the repair")
    mf.close()
    guards.closed("after the repair")


def test_damage_of_a_freed_buffer_is_remembered_until_reset(bbme, guards):
    from test_gpu_context_state import _hip
    hip = _hip()
    f1, f2, _ = bbme.synth_pair(128, 96, 2, max_motion=2)
    mf = guards.own(bbme.MF(f1, f2, [20], [8]))
    band = C.c_void_p()
    guards.capi.check(guards.lib.bbme_test_guard_find(b"work buffers", 1, C.byref(band)))
    new = (C.c_ubyte * 2)(0, 0)
    assert hip.hipMemcpy(band.value + 100, C.addressof(new), 2, 1) == 0
    mf.close()
    live, violations, first = guards.check()
    assert live == guards.base_live and violations == 1 and "back guard, offset 100 from" in first and "(2 damaged bytes" in first, first
    guards.capi.check(guards.lib.bbme_test_guard_reset())
    guards.closed("after the reset")


def test_poison_is_in_the_slack_of_an_uploaded_table(bbme, guards):
    """The poison knob did something: the 64 bytes of slack behind level 0's rank table ("search plan of level 0" is first the text
    of Level::rank_of) hold the poison pattern, read back from in front of the buffer's back guard."""
    from test_gpu_context_state import _hip
    hip = _hip()
    f1, f2, _ = bbme.synth_pair(128, 96, 3, max_motion=2)
    mf = guards.own(bbme.MF(f1, f2, [20, 20], [8, 8]))
    band = C.c_void_p()
    guards.capi.check(guards.lib.bbme_test_guard_find(b"search plan of level 0", 1, C.byref(band)))
    slack = (C.c_ubyte * 64)()
    assert hip.hipMemcpy(C.addressof(slack), band.value - 64, 64, 2) == 0                # 2: device to host
    assert bytes(slack) == b"\xc7" * 64, bytes(slack).hex()
    mf.close()
    guards.closed("poisoned slack")


def test_find_needs_the_knob(bbme, monkeypatch):
    from blockbasedmotionestimation_amd import _capi
    monkeypatch.delenv("BBME_TEST_GUARD", raising=False)
    band = C.c_void_p()
    assert _capi.lib().bbme_test_guard_find(b"work buffers", 1, C.byref(band)) == _capi.ERR_UNSUPPORTED
    assert not band.value
