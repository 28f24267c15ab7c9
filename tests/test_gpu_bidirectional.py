"""Direction, bidirectional estimate and forward-backward consistency on the GPU (include/bbme.h): a context in direction
BACKWARD is bit for bit a context fed the exchanged pair and the oracle's OracleMF(f2, f1); bbme_estimate_bidirectional leaves
both fields of every pair from planes set once; k_fb_consistency gives exactly the numpy restatement of the rule
(test_consistency_cpu.np_cells_consistency) on the oracle's two grids and on injected grids with targets outside the plane and
int16 extremes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _odd_window, _stats_of, _write_pgm, assert_stages_equal, gpu_schedule, oracle_schedule
from test_consistency_cpu import (GENERATORS, STAT_KEYS, TOLS, np_cells_consistency, windows_of)

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu

# name: (source width, height, search, block, seed, max motion, upsample) -- the table of tests/test_gpu_motion_compensation.py
CASES = {
    "cfg1_like": (200, 136, [30] * 3, [16] * 3, 601, 7, 1),
    "ref2": (376, 250, [32, 32, 42], [16, 16, 32], 602, 10, 1),
    "b8_r32": (160, 96, [72, 72], [8, 8], 603, 24, 1),
    "block2": (160, 128, [12, 20], [2, 4], 604, 4, 1),
    "x4": (48, 36, [30, 30], [16, 16], 605, 3, 4),
    "border_motion": (128, 96, [48, 48], [16, 16], 606, 24, 1),
}


# (consistent, inconsistent) cells of the oracle's two fields: forward mask, tolerance 1, default window
ORACLE_TOL1 = {"cfg1_like": (5690, 1110), "ref2": (20098, 3402), "b8_r32": (1961, 1879), "block2": (4526, 594), "x4": (3250, 3662),
               "border_motion": (2407, 665)}
# inconsistent cells of synth_video(200, 136, 5, 77, max_motion=6)'s four pairs: forward, tolerance 1, all 12 288 cells
ORACLE_VIDEO_TOL1 = [2482, 1809, 2580, 1688]


def _frames(bbme, name):
    w, h, _, _, seed, mm, _ = CASES[name]
    f1, f2, _ = bbme.synth_pair(w, h, seed, max_motion=mm)
    if name == "border_motion":
        # one global motion (5, 3): blocks at the right and bottom edges whose MV the larger blocks inherit point outside
        f2 = np.roll(f1, (3, 5), axis=(0, 1))
    return f1, f2


_ORACLE = {}


def _oracle_fields(bbme, oracle, f1, f2, search, block, upsample=1, raster=False, key=None):
    """(flow, cells (CH, CW, 2) int16) of the oracle's whole schedule on (f1, f2); cached per `key`."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    if upsample == 4:
        f1, f2 = bbme.resize_x4(f1), bbme.resize_x4(f2)
    omf = oracle.OracleMF(f1, f2, search, block)
    if raster:
        omf.set_raster_search(True)
    flow = oracle_schedule(omf, len(block))
    cells = omf.block_mvs(0, 2).astype(np.int16)
    omf.close()
    if key is not None:
        _ORACLE[key] = (flow, cells)
    return flow, cells


def _both_oracles(bbme, oracle, name):
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    fwd = _oracle_fields(bbme, oracle, f1, f2, search, block, up, key=(name, "f"))
    bwd = _oracle_fields(bbme, oracle, f2, f1, search, block, up, key=(name, "b"))
    return fwd, bwd


def _blocks(B):
    b = 1
    while b <= B:
        yield b
        b *= 2


def _results(mf, levels, blocks):
    """Everything a direction must agree on with the context of the exchanged pair."""
    out = dict(flow=mf.get_flow(), cells=mf.get_cells(), sub=mf.get_subsampled_flow(), sub4=mf.get_subsampled_flow(4),
               err=mf.compensation_error())
    for lvl in range(levels):
        for b in _blocks(blocks[lvl]):
            out["mc", lvl, b] = mf.draw_MVimage(lvl, b, 7)
            out["err", lvl, b] = mf.compensation_error(lvl, b)
    return out


def _assert_same(got, exp, what):
    assert got.keys() == exp.keys()
    for k in exp:
        if isinstance(exp[k], np.ndarray):
            assert np.array_equal(got[k], exp[k]), (what, k)
        else:
            assert got[k] == exp[k], (what, k)


MODES = {
    "default": ({}, None),
    "no_graph": ({"BBME_NO_GRAPH": "1"}, None),
    "no_speculation": ({}, "speculation_off"),
    "speculate_every_level": ({"BBME_SPEC_MIN_GABS": "0", "BBME_SPECULATE": "1"}, None),
    # both directions' graphs with the speculative branch (by default a context keeps one such graph)
    "both_graphs_forked": ({"BBME_SPEC_MIN_GABS": "0", "BBME_SPECULATE": "1", "BBME_SPECULATE_BOTH_GRAPHS": "1"}, None),
}


def _make(bbme, monkeypatch, env, *args, **kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return bbme.MF(*args, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_direction_backward_is_the_exchanged_pair(bbme, oracle, monkeypatch, name, mode):
    _, _, search, block, _, _, up = CASES[name]
    env, switch = MODES[mode]
    f1, f2 = _frames(bbme, name)
    (oflow_f, _), (oflow_b, ocells_b) = _both_oracles(bbme, oracle, name)
    L = len(block)
    mf = _make(bbme, monkeypatch, env, f1, f2, search, block, upsample=up)
    ex = _make(bbme, monkeypatch, env, f2, f1, search, block, upsample=up)
    if switch == "speculation_off":
        mf.set_speculation(False)
        ex.set_speculation(False)
    assert mf.direction == bbme.DIR_FORWARD
    planes = [mf.get_level_planes(l) for l in range(L)]
    mf.set_direction(True)
    assert mf.direction == bbme.DIR_BACKWARD
    mf.estimate_async()
    ex.estimate_async()
    got = _results(mf, L, block)
    _assert_same(got, _results(ex, L, block), "backward")
    assert np.array_equal(got["flow"], oflow_b)
    assert np.array_equal(got["cells"], ocells_b)
    for l in range(L):                                           # the direction moves no plane
        a, b = mf.get_level_planes(l)
        assert np.array_equal(a, planes[l][0]) and np.array_equal(b, planes[l][1]), l
    mf.set_direction(True)                                       # the direction it has: nothing changes
    assert np.array_equal(mf.get_cells(), ocells_b)
    mf.set_direction(False)
    mf.estimate_async()
    assert np.array_equal(mf.get_flow(), oflow_f)
    # alternating re-uses each direction's graph; every estimate is the oracle's
    for back in (True, False, True):
        mf.set_direction(back)
        mf.estimate_async()
        assert np.array_equal(mf.get_flow(), oflow_b if back else oflow_f), back
    mf.close()
    ex.close()


@pytest.mark.parametrize("name", ["cfg1_like", "b8_r32"])
def test_direction_with_raster_search_and_jacobi_sweeps(bbme, oracle, name):
    _, _, search, block, _, _, up = CASES[name]
    f1, f2 = _frames(bbme, name)
    L = len(block)
    for which in ("raster", "jacobi"):
        mf = bbme.MF(f1, f2, search, block, upsample=up)
        ex = bbme.MF(f2, f1, search, block, upsample=up)
        for m in (mf, ex):
            if which == "raster":
                m.set_search_mode(True)
            else:
                m.set_regularizer_mode(True)
        mf.set_direction(True)
        mf.estimate_async()
        ex.estimate_async()
        got = _results(mf, L, block)
        _assert_same(got, _results(ex, L, block), which)
        if which == "raster":
            oflow, _ = _oracle_fields(bbme, oracle, f2, f1, search, block, up, raster=True)
            assert np.array_equal(got["flow"], oflow)
        fwd = bbme.MF(f1, f2, search, block, upsample=up)
        if which == "raster":
            fwd.set_search_mode(True)
        else:
            fwd.set_regularizer_mode(True)
        fwd.estimate_async()
        mf.set_direction(False)
        mf.estimate_async()
        assert np.array_equal(mf.get_flow(), fwd.get_flow()), which
        assert not np.array_equal(mf.get_flow(), got["flow"]), which
        for m in (mf, ex, fwd):
            m.close()


@pytest.mark.parametrize("name", ["cfg1_like", "border_motion"])
def test_stage_by_stage_in_direction_backward(bbme, oracle, name):
    from blockbasedmotionestimation_amd import _capi
    _, _, search, block, _, _, _ = CASES[name]
    f1, f2 = _frames(bbme, name)
    L = len(block)
    omf = oracle.OracleMF(f2, f1, search, block)
    mf = bbme.MF(f1, f2, search, block)
    mf.estimate_async()
    mf.synchronize()
    # the oracle's planes in their PHYSICAL roles: the product's image 1 is the oracle's image 2
    for lvl in range(L):
        mf.set_level_planes(lvl, omf.image(lvl, 2), omf.image(lvl, 1))
    mf.set_direction(True)
    for call in (lambda: mf.draw_MVimage(0, 2), lambda: mf.compensation_error(L - 1, block[-1]), mf.get_cells,
                 mf.get_subsampled_flow):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == _capi.ERR_STATE
    exp = []
    oflow = oracle_schedule(omf, L, lambda *a: exp.append(a))
    got = []
    gflow = gpu_schedule(mf, L, block, lambda *a: got.append(a))
    assert_stages_equal(exp, got, name)
    assert np.array_equal(gflow, oflow)
    omf.close()
    mf.close()


def _check_bidirectional(bbme, mf, fwd, bwd, what, name=None):
    (oflow_f, ocells_f), (_, ocells_b) = fwd, bwd
    assert mf.direction == bbme.DIR_FORWARD, what
    assert np.array_equal(mf.get_flow(), oflow_f), what
    assert np.array_equal(mf.get_cells(), ocells_f), what
    assert np.array_equal(mf.get_backward_cells(), ocells_b), what
    CH, CW = ocells_f.shape[:2]
    assert mf.cells_shape == (CH, CW)
    default = mf.default_cell_window()
    px, py = mf.padding_x, mf.padding_y
    assert default == (-(-px // 2), -(-py // 2), -(-(px + mf.orig_width) // 2) - -(-px // 2),
                       -(-(py + mf.orig_height) // 2) - -(-py // 2))
    for which, (a, b) in (("forward", (ocells_f, ocells_b)), ("backward", (ocells_b, ocells_f))):
        for tol in (0, 1, 2):
            exp_mask, _ = np_cells_consistency(a, b, tol)
            assert np.array_equal(mf.consistency(which, tol), exp_mask), (what, which, tol)
            for window, arg in (((0, 0, CW, CH), "all"), (default, None), (_odd_window(mf), _odd_window(mf))):
                _, exp = np_cells_consistency(a, b, tol, window)
                print("%s %s tol %d window %s: %s" % (what, which, tol, window, exp))
                assert _stats(mf.consistency_stats(which, tol, arg)) == exp, (what, which, tol, window)
                if arg is None:
                    # non-degenerate content: neither class is rare, and no estimated vector leaves the plane
                    n = window[2] * window[3]
                    assert exp[2] == 0 and exp[0] + exp[1] == n
                    assert min(exp[0], exp[1]) * 20 >= n, (what, which, tol, exp)
                    if name and which == "forward" and tol == 1:
                        assert exp[:2] == ORACLE_TOL1[name]


@pytest.mark.parametrize("name", list(CASES))
def test_bidirectional_estimate(bbme, oracle, name):
    _, _, search, block, seed, mm, up = CASES[name]
    w, h = CASES[name][:2]
    f1, f2 = _frames(bbme, name)
    fwd, bwd = _both_oracles(bbme, oracle, name)
    plain = bbme.MF(f1, f2, search, block, upsample=up)
    plain.estimate_async()
    mf = bbme.MF(f1, f2, search, block, upsample=up)
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.get_flow(), plain.get_flow()) and np.array_equal(mf.get_cells(), plain.get_cells())
    plain.close()
    _check_bidirectional(bbme, mf, fwd, bwd, name, name)
    mf.estimate_bidirectional_async()                            # the same call again on the same context
    _check_bidirectional(bbme, mf, fwd, bwd, name + " again")
    mf.set_direction(True)                                       # from direction BACKWARD: still leaves FORWARD
    mf.estimate_bidirectional_async()
    _check_bidirectional(bbme, mf, fwd, bwd, name + " from backward")
    # a long-lived context: another pair of the same size, then the first again (a stale SAD memo would show here)
    g1, g2, _ = bbme.synth_pair(w, h, seed + 50, max_motion=mm)
    mf.set_frames(g1, g2)
    mf.estimate_bidirectional_async()
    other = (_oracle_fields(bbme, oracle, g1, g2, search, block, up), _oracle_fields(bbme, oracle, g2, g1, search, block, up))
    assert np.array_equal(mf.get_flow(), other[0][0])
    assert np.array_equal(mf.get_cells(), other[0][1]) and np.array_equal(mf.get_backward_cells(), other[1][1])
    mf.set_frames(f1, f2)
    mf.estimate_bidirectional_async()
    _check_bidirectional(bbme, mf, fwd, bwd, name + " after another pair")
    mf.close()


def test_identical_frames_are_consistent_everywhere(bbme, oracle):
    f1, _, _ = bbme.synth_pair(200, 136, 611, max_motion=7)
    search, block = [30] * 3, [16] * 3
    _, ocells = _oracle_fields(bbme, oracle, f1, f1, search, block)
    assert not ocells.any()
    mf = bbme.MF(f1, f1.copy(), search, block)
    mf.estimate_bidirectional_async()
    assert not mf.get_cells().any() and not mf.get_backward_cells().any()
    CH, CW = mf.cells_shape
    for which in ("forward", "backward"):
        assert not mf.consistency(which, 0).any()
        assert _stats(mf.consistency_stats(which, 0, "all")) == (CH * CW, 0, 0, 0)
    mf.close()


def _device_consistency(bbme, mf, a, b, tol, window, mask=True, stats=True, stream=None, extra=0):
    import torch
    CH, CW = mf.cells_shape
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    big = torch.full((CH, CW + extra), 0xAB, dtype=torch.uint8, device="cuda") if mask else None
    st = torch.full((4,), -1, dtype=torch.int64, device="cuda") if stats else None
    torch.cuda.synchronize()
    mf.cells_consistency_device(ta, tb, tol, big[:, :CW] if mask else None, st, window, stream.cuda_stream if stream else None)
    if stream:
        stream.synchronize()
    else:
        mf.synchronize()
    got = big.cpu().numpy() if mask else None
    return got, (tuple(int(v) for v in st.cpu().numpy()) if stats else None)


# (source width, height, search, block): cell grids of 24 x 32, 26 x 38 (CW not a multiple of 4) and 34 x 50
INJECT_GEOMETRIES = [(64, 48, [12], [4]), (76, 52, [12], [4]), (100, 68, [12], [4])]


@pytest.mark.parametrize("geom", range(len(INJECT_GEOMETRIES)))
@pytest.mark.parametrize("kind", list(GENERATORS))
def test_injected_grids_on_the_device(bbme, kind, geom):
    import torch
    w, h, search, block = INJECT_GEOMETRIES[geom]
    z = np.zeros((h, w), np.uint8)
    mf = bbme.MF(z, z, search, block)                             # no estimate: the device call needs none
    assert (mf.padding_x, mf.padding_y) == (0, 0)
    CH, CW = mf.cells_shape
    assert (CH, CW) == (h // 2, w // 2)
    rng = np.random.default_rng(1000 * CH + CW + len(kind))
    a, b = GENERATORS[kind](CH, CW, rng)
    side = torch.cuda.Stream()
    seen = set()
    for tol in TOLS:
        for window in windows_of(CH, CW):
            exp_mask, exp = np_cells_consistency(a, b, tol, window)
            got, st = _device_consistency(bbme, mf, a, b, tol, window)
            assert np.array_equal(got, exp_mask), (tol, window)
            assert st == exp, (tol, window)
        seen |= set(np.unique(exp_mask).tolist())
        exp_mask, exp = np_cells_consistency(a, b, tol)
        # a column slice of a wider tensor with an odd pitch (and an aligned one) on a side stream: the bytes beside it stay
        for extra in (13, 16):
            got, st = _device_consistency(bbme, mf, a, b, tol, None, stream=side, extra=extra)
            assert np.array_equal(got[:, :CW], exp_mask) and (got[:, CW:] == 0xAB).all() and st == exp, (tol, extra)
        got, st = _device_consistency(bbme, mf, a, b, tol, None, stats=False, extra=13)
        assert np.array_equal(got[:, :CW], exp_mask) and (got[:, CW:] == 0xAB).all() and st is None
        got, st = _device_consistency(bbme, mf, a, b, tol, None, mask=False)
        assert got is None and st == exp
    if kind != "small":
        assert 2 in seen
    if kind == "extreme":
        assert seen == {0, 1, 2}
    # uint64 statistics too
    st = torch.zeros(4, dtype=torch.uint64, device="cuda")
    mf.cells_consistency_device(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), 1, None, st)
    mf.synchronize()
    assert tuple(int(v) for v in st.cpu().numpy().astype(np.uint64)) == np_cells_consistency(a, b, 1)[1]
    mf.close()


def _single_bidirectional(bbme, f1, f2, search, block):
    mf = bbme.MF(f1, f2, search, block)
    mf.estimate_bidirectional_async()
    out = dict(cells=mf.get_cells(), back=mf.get_backward_cells(),
               masks={(w, t): mf.consistency(w, t) for w in ("forward", "backward") for t in (0, 1)},
               stats={(w, t, win): mf.consistency_stats(w, t, win) for w in ("forward", "backward") for t in (0, 1)
                      for win in (None, "all")})
    mf.close()
    return out


def _check_pairs_against_singles(mb, singles, what):
    for p, s in enumerate(singles):
        assert np.array_equal(mb.get_pair_cells(p), s["cells"]), (what, p)
        assert np.array_equal(mb.get_pair_backward_cells(p), s["back"]), (what, p)
        for (w, t), m in s["masks"].items():
            assert np.array_equal(mb.consistency(w, t, pair=p), m), (what, p, w, t)
    for w in ("forward", "backward"):
        for t in (0, 1):
            for win in (None, "all"):
                got = mb.consistency_stats_all(w, t, win)
                assert got == [s["stats"][w, t, win] for s in singles], (what, w, t, win)
    assert mb.consistency_stats() == singles[0]["stats"]["forward", 1, None]


def _assert_state_errors(bbme, mb, what):
    from blockbasedmotionestimation_amd import _capi
    import torch
    calls = [mb.get_backward_cells, lambda: mb.consistency("forward", 1), lambda: mb.consistency_stats(),
             lambda: mb.backward_cells_device_ptr(0)]
    if isinstance(mb, bbme.MFBatch):
        calls += [lambda: mb.get_pair_backward_cells(mb.batch - 1), lambda: mb.consistency_stats_all("backward", 0),
                  lambda: mb.consistency("backward", 0, pair=mb.batch - 1)]
    for call in calls:
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == _capi.ERR_STATE, what
    CH, CW = mb.cells_shape
    z = torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    mb.cells_consistency_device(z, z, 0, None, st)                # needs no valid pair of fields
    torch.cuda.synchronize()
    assert tuple(st.cpu().tolist()) == (CH * CW, 0, 0, 0), what


def test_batch_equals_single_contexts(bbme):
    search, block = [30, 30, 30], [16, 16, 16]
    pairs = [bbme.synth_pair(200, 136, 700 + i, max_motion=6 + 4 * i)[:2] for i in range(3)]
    singles = [_single_bidirectional(bbme, p[0], p[1], search, block) for p in pairs]
    mb = bbme.MFBatch(pairs, search, block)
    _assert_state_errors(bbme, mb, "before any estimate")
    mb.estimate_bidirectional_async()
    _check_pairs_against_singles(mb, singles, "batch")
    counts = [s["stats"]["forward", 1, "all"]["inconsistent"] for s in singles]
    assert len(set(counts)) > 1
    # every invalidating call
    mb.estimate_async()
    _assert_state_errors(bbme, mb, "estimate")
    mb.estimate_bidirectional_async()
    mb.set_direction(True)
    _assert_state_errors(bbme, mb, "set_direction")
    mb.set_direction(False)
    _assert_state_errors(bbme, mb, "set_direction back")
    mb.estimate_bidirectional_async()
    mb.set_direction(False)                                      # the direction it has: still valid
    _check_pairs_against_singles(mb, singles, "batch again")
    mb.set_pair(1, *pairs[1])
    _assert_state_errors(bbme, mb, "set_pair")
    mb.estimate_bidirectional_async()
    _check_pairs_against_singles(mb, singles, "batch after set_pair")
    mb.close()


def test_single_context_invalidating_calls(bbme):
    f1, f2, _ = bbme.synth_pair(200, 136, 901, max_motion=7)
    search, block = [30] * 3, [16] * 3
    mf = bbme.MF(f1, f2, search, block)
    single = _single_bidirectional(bbme, f1, f2, search, block)
    planes = mf.get_level_planes(1)
    for what, call in (("set_frames", lambda: mf.set_frames(f1, f2)),
                       ("set_level_planes", lambda: mf.set_level_planes(1, *planes)),
                       ("estimate", mf.estimate_async),
                       ("stage_search", lambda: mf.stage_search(2)),
                       ("stage_regularize", lambda: mf.stage_regularize(2, 2, 1)),
                       ("stage_set_mvs", lambda: mf.stage_set_mvs(2, 2, mf.stage_get_mvs(2, 2)))):
        mf.estimate_bidirectional_async()
        assert np.array_equal(mf.get_backward_cells(), single["back"]), what
        mf.get_level_planes(0)                                   # reading planes invalidates nothing
        mf.stage_expand()
        assert np.array_equal(mf.consistency("forward", 1), single["masks"]["forward", 1]), what
        call()
        _assert_state_errors(bbme, mf, what)
    mf.close()


def test_chain_equals_single_contexts(bbme):
    from blockbasedmotionestimation_amd import _capi
    search, block = [30, 30, 30], [16, 16, 16]
    video = bbme.synth_video(200, 136, 5, 77, max_motion=6)
    singles = [_single_bidirectional(bbme, video[p], video[p + 1], search, block) for p in range(4)]
    counts = [s["stats"]["forward", 1, "all"]["inconsistent"] for s in singles]
    assert counts == ORACLE_VIDEO_TOL1                                           # of 12 288 cells: not degenerate
    chain = bbme.MFChain(video[0:3], search, block)
    chain.estimate_bidirectional_async()
    _check_pairs_against_singles(chain, singles[0:2], "chain round 0")
    # direction BACKWARD on a chain: pair p = (slot p + 1, slot p)
    chain.set_direction(True)
    _assert_state_errors(bbme, chain, "chain set_direction")
    chain.estimate_async()
    for p in range(2):
        assert np.array_equal(chain.get_pair_cells(p), singles[p]["back"]), p
    chain.set_direction(False)
    chain.estimate_bidirectional_async()
    _check_pairs_against_singles(chain, singles[0:2], "chain round 0 again")
    chain.advance([video[3]])
    _assert_state_errors(bbme, chain, "between advance and the last slot")
    with pytest.raises(bbme.BbmeError) as e:
        chain.estimate_bidirectional_async()
    assert e.value.status == _capi.ERR_STATE
    chain.set_frame_run(2, [video[4]])
    _assert_state_errors(bbme, chain, "slots set, not estimated")
    chain.estimate_bidirectional_async()
    _check_pairs_against_singles(chain, singles[2:4], "chain round 1")
    chain.close()


def test_consistency_calls_change_no_state_and_refuse_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    f1, f2, _ = bbme.synth_pair(200, 136, 901, max_motion=7)
    search, block = [30] * 3, [16] * 3
    mf = bbme.MF(f1, f2, search, block)
    mf.estimate_bidirectional_async()
    before = dict(flow=mf.get_flow(), cells=mf.get_cells(), back=mf.get_backward_cells(), mc=mf.draw_MVimage(),
                  err=mf.compensation_error(), sub=mf.get_subsampled_flow(4))
    CH, CW = mf.cells_shape
    ta = torch.from_numpy(before["cells"]).cuda()
    tb = torch.from_numpy(before["back"]).cuda()
    mask = torch.zeros((CH, CW), dtype=torch.uint8, device="cuda")
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    results = []
    for which in ("forward", "backward"):
        for tol in (0, 1, 2):
            results.append(mf.consistency(which, tol))
            results.append(mf.consistency_stats(which, tol))
            results.append(mf.consistency_stats(which, tol, "all"))
    mf.cells_consistency_device(ta, tb, 1, mask, st)
    mf.synchronize()
    assert np.array_equal(mask.cpu().numpy(), mf.consistency("forward", 1))
    assert tuple(st.cpu().tolist()) == _stats(mf.consistency_stats("forward", 1, "all"))
    # the context's own backward cells in HBM are what the getter downloads
    p = C.c_void_p()
    assert L.bbme_cells_device_pair(mf._ctx, 0, C.byref(p)) == 0
    assert L.bbme_cells_consistency_device(mf._ctx, p, C.c_void_p(mf.backward_cells_device_ptr()), 2, None,
                                           C.c_void_p(mask.data_ptr()), CW, None, None) == 0
    mf.synchronize()
    assert np.array_equal(mask.cpu().numpy(), mf.consistency("forward", 2))
    # the other getters' scratch buffers and the consistency's are independent
    m1 = mf.consistency("forward", 1)
    mf.draw_MVimage()
    mf.compensation_error()
    mf.get_subsampled_flow(1)
    assert np.array_equal(mf.consistency("forward", 1), m1)
    after = dict(flow=mf.get_flow(), cells=mf.get_cells(), back=mf.get_backward_cells(), mc=mf.draw_MVimage(),
                 err=mf.compensation_error(), sub=mf.get_subsampled_flow(4))
    _assert_same(after, before, "no state change")
    # argument errors
    ctx, inv = mf._ctx, _capi.ERR_INVALID
    buf = np.zeros((CH, CW), np.uint8)
    s4 = (C.c_ulonglong * 4)()
    d = C.c_int()
    p = C.c_void_p()
    assert L.bbme_set_direction(ctx, 2) == inv and L.bbme_set_direction(ctx, -1) == inv
    assert L.bbme_get_direction(ctx, None) == inv
    assert L.bbme_get_direction(ctx, C.byref(d)) == 0 and d.value == 0
    for pair in (-1, 1):
        assert L.bbme_backward_cells_device_pair(ctx, pair, C.byref(p)) == inv
        assert L.bbme_get_backward_cells_host_pair(ctx, pair, buf.ctypes.data) == inv
        assert L.bbme_get_consistency_host(ctx, pair, 0, 1, buf.ctypes.data) == inv
    assert L.bbme_backward_cells_device_pair(ctx, 0, None) == inv
    assert L.bbme_get_backward_cells_host_pair(ctx, 0, None) == inv
    assert L.bbme_get_consistency_host(ctx, 0, 0, 1, None) == inv
    for which in (-1, 2):
        assert L.bbme_get_consistency_host(ctx, 0, which, 1, buf.ctypes.data) == inv
        assert L.bbme_consistency_stats(ctx, which, 1, None, s4) == inv
    assert L.bbme_get_consistency_host(ctx, 0, 0, -1, buf.ctypes.data) == inv
    assert L.bbme_consistency_stats(ctx, 0, -1, None, s4) == inv
    assert L.bbme_consistency_stats(ctx, 0, 1, None, None) == inv
    a_, b_, m_, s_ = (C.c_void_p(t.data_ptr()) for t in (ta, tb, mask, st))
    assert L.bbme_cells_consistency_device(ctx, None, b_, 1, None, m_, CW, s_, None) == inv
    assert L.bbme_cells_consistency_device(ctx, a_, None, 1, None, m_, CW, s_, None) == inv
    assert L.bbme_cells_consistency_device(ctx, a_, b_, 1, None, None, CW, None, None) == inv
    assert L.bbme_cells_consistency_device(ctx, a_, b_, -1, None, m_, CW, s_, None) == inv
    assert L.bbme_cells_consistency_device(ctx, a_, b_, 1, None, m_, CW - 1, s_, None) == inv
    for win in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (CW - 7, 0, 8, 8), (0, CH - 7, 8, 8), (0, 0, CW + 1, CH)):
        w4 = (C.c_int * 4)(*win)
        assert L.bbme_consistency_stats(ctx, 0, 1, w4, s4) == inv, win
        assert L.bbme_cells_consistency_device(ctx, a_, b_, 1, w4, m_, CW, s_, None) == inv, win
    assert L.bbme_consistency_stats(ctx, 0, 1, (C.c_int * 4)(CW - 8, CH - 8, 8, 8), s4) == 0
    with pytest.raises(bbme.BbmeError) as e:
        mf.consistency("sideways")
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.cells_consistency_device(ta[:, :CW - 2], tb, 1, mask, st)
    assert e.value.status == inv
    _assert_same(dict(flow=mf.get_flow(), back=mf.get_backward_cells()), dict(flow=before["flow"], back=before["back"]), "errors")
    mf.close()


def test_cli_writes_the_backward_field_and_the_occlusion_mask(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    f1, f2, _ = bbme.synth_pair(96, 72, 1001, max_motion=3)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    args = ["--levels", "3", "--block", "16", "--search", "30"]
    base = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm")] + args
    r0 = subprocess.run(base + ["--out", str(tmp_path / "a.flo"), "--color", str(tmp_path / "a.ppm")], capture_output=True,
                        text=True, timeout=300)
    assert r0.returncode == 0, r0.stderr
    r1 = subprocess.run(base + ["--out", str(tmp_path / "b.flo"), "--color", str(tmp_path / "b.ppm"), "--backward",
                                str(tmp_path / "back.flo"), "--occlusion", str(tmp_path / "occ.pgm")], capture_output=True,
                        text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr
    assert (tmp_path / "a.flo").read_bytes() == (tmp_path / "b.flo").read_bytes()
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    assert "consistent" not in r0.stdout
    assert [l for l in r0.stdout.splitlines() if not l.startswith("Seconds")] == \
           [l for l in r1.stdout.splitlines() if not l.startswith("Seconds") and not l.startswith("consistent")]
    mf = bbme.MF(f1, f2, [30] * 3, [16] * 3, upsample=4)
    mf.estimate_bidirectional_async()
    fwd_sub = mf.get_subsampled_flow()
    mask = mf.consistency("forward", 1)
    st = mf.consistency_stats("forward", 1)
    cx0, cy0, cw, ch = mf.default_cell_window()
    lut = np.array([0, 128, 255], np.uint8)
    assert (tmp_path / "occ.pgm").read_bytes() == b"P5\n%d %d\n255\n" % (cw, ch) + lut[mask[cy0:cy0 + ch, cx0:cx0 + cw]].tobytes()
    assert "consistent %d inconsistent %d outside %d\n" % (st["consistent"], st["inconsistent"], st["outside"]) in r1.stdout
    assert st["consistent"] + st["inconsistent"] + st["outside"] == cw * ch and st["inconsistent"] > 0
    mf.set_direction(True)
    mf.estimate_async()
    back_sub = mf.get_subsampled_flow()
    mf.close()
    flow = bbme.Flow()
    assert np.array_equal(np.asarray(flow.ReadFlowFile(str(tmp_path / "back.flo"))), back_sub)
    assert np.array_equal(np.asarray(flow.ReadFlowFile(str(tmp_path / "a.flo"))), fwd_sub)
    assert not np.array_equal(back_sub, fwd_sub)
    r = subprocess.run([_build.CLI], capture_output=True, text=True)
    assert r.returncode == 2 and "--backward" in r.stderr and "--occlusion" in r.stderr


def test_estimate_frames_bidirectional(bbme):
    from blockbasedmotionestimation_amd.sequence import estimate_frames_bidirectional, estimate_frames_pipelined, expand_cells_host
    search, block = [30, 30, 30], [16, 16, 16]
    video = bbme.synth_video(200, 136, 7, 78, max_motion=6)
    got = estimate_frames_bidirectional(video, search, block, in_flight=4, batch=2)
    plain = estimate_frames_pipelined(video, search, block, in_flight=4, batch=2)
    assert len(got) == len(plain) == 6
    for p in range(6):
        mf = bbme.MF(video[p], video[p + 1], search, block)
        mf.estimate_bidirectional_async()
        h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
        cx0, cy0, cw, ch = mf.default_cell_window()
        fwd = mf.get_flow()[py:py + h, px:px + w]
        bwd = expand_cells_host(mf.get_backward_cells().view(np.int32)[..., 0])[py:py + h, px:px + w]
        assert np.array_equal(got[p][0], fwd) and np.array_equal(got[p][0], plain[p]), p
        assert np.array_equal(got[p][1], bwd), p
        for k, which in ((2, "forward"), (3, "backward")):
            assert np.array_equal(got[p][k], mf.consistency(which, 1)[cy0:cy0 + ch, cx0:cx0 + cw]), (p, which)
            assert got[p][k].shape == (ch, cw) and got[p][k].dtype == np.uint8
        mf.set_direction(True)
        mf.estimate_async()
        assert np.array_equal(got[p][1], mf.get_flow()[py:py + h, px:px + w]), p
        mf.close()
