"""The kernels at the limits of their packed sums, keys and vectors, against the CPU oracle bit for bit and stage by stage.
The content comes from helpers.py and is proven to do what these tests need in tests/test_limits_cpu.py: block SADs at the
ceiling 255 B^2 (the u16 lanes of the packed accumulators, the (SAD, rank) keys), winners on the outermost ring of the spiral,
energies beyond 2^24 (float32 no longer exact), vectors at the bounds of the memo's 14-bit packing and of int16, and the two
reductions (compensation statistics, EPE) at saturation.  Expected values come from the oracle, numpy or closed-form integers
at run time."""
import contextlib
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def knobs(env):
    """The environment a context is created under (the library reads its knobs in bbme_create_batch)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


_expected = {}


def expected_stages(oracle, name):
    """The oracle's schedule on a content, computed once per session (several forms of the product run on each)."""
    if name not in _expected:
        c = H.LIMIT_CONTENTS[name]
        p1, p2 = H.limit_content_planes(name)
        _expected[name] = (p1, p2, H.oracle_stages_from_planes(oracle, p1, p2, c["search"], c["block"], c["raster"]))
    return _expected[name]


def _env_id(env):
    return ",".join("%s=%s" % (k.replace("BBME_", "").lower(), v) for k, v in sorted(env.items())) or "default"


# ---- 2. every SAD path at that content --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env", H.LIMIT_SEARCH_CASES, ids=["%s-%s" % (n, _env_id(e)) for n, e in H.LIMIT_SEARCH_CASES])
def test_search_forms_at_the_ceiling(bbme, oracle, name, env):
    """k_search_fast<8|16|32, 1|2> under the tight and the loose plan, even ranges, odd shifts, R = 63; k_search_generic for blocks
    of 2, 4 and 64, ranges of 64 and 127, forced onto B = 16 / 32, and in raster mode; followed by the default sweeps from B down
    to 2.  Every grid against the oracle's."""
    c = H.LIMIT_CONTENTS[name]
    p1, p2, exp = expected_stages(oracle, name)
    with knobs(env):
        H.gpu_stages_match(bbme, p1, p2, c["search"], c["block"], exp, c["raster"], what="%s %s" % (name, env))


@pytest.mark.parametrize("form", list(H.LIMIT_REG_FORMS))
@pytest.mark.parametrize("name", H.LIMIT_REG_CONTENTS)
def test_regulariser_forms_at_the_ceiling(bbme, oracle, name, form):
    """Every form of the regulariser's SAD paths (strip pass 1, chain / throughput pass 1, one-wave workgroups and a one-wave solver, forced relaxation
    launches, the memo off, on from b = 8 with and without forwarding) over all block sizes from B down to 2."""
    c = H.LIMIT_CONTENTS[name]
    env = H.LIMIT_REG_FORMS[form]
    p1, p2, exp = expected_stages(oracle, name)
    memo = {"lookups": 0, "misses": 0}

    def probe(mf, stage, level, b):
        if stage.startswith("sweep"):
            st = mf.sweep_stats()
            memo["lookups"] += st[9]
            memo["misses"] += st[10]
    with knobs(env):
        H.gpu_stages_match(bbme, p1, p2, c["search"], c["block"], exp, c["raster"], what="%s %s" % (name, form), probe=probe)
    print("%s %s: memo lookups %d misses %d" % (name, form, memo["lookups"], memo["misses"]))
    if form == "memo_off":
        assert memo["lookups"] == 0
    elif form.startswith("memo_b8"):
        assert memo["lookups"] > 0, "the SAD memo was never looked up: the case passed by bypassing the path"


@pytest.mark.parametrize("list_split", ["0", "1"])
@pytest.mark.parametrize("split", ["0", "100000000"])
@pytest.mark.parametrize("name", H.LIMIT_SPEC_CONTENTS)
def test_speculative_search_and_list_kernel_at_the_ceiling(bbme, oracle, name, split, list_split):
    """bbme_estimate with the speculative search forced onto every level: k_search_fast in its speculative mode, k_fixup_list and
    k_search_list<B, 1|2>.  The final field and every level's final grid against the oracle, twice on one context."""
    c = H.LIMIT_CONTENTS[name]
    p1, p2, (_, oflow, finals) = expected_stages(oracle, name)
    with knobs({"BBME_SPEC_MIN_GABS": "0", "BBME_SPECULATE": "1", "BBME_LIST_SPLIT": list_split, "BBME_SEARCH_SPLIT_BLOCKS": split}):
        mf = H.make_mf_from_planes(bbme, p1, p2, c["search"], c["block"])
    mf.set_speculation(True)
    for run in range(2):
        flow = mf.calcMotionBlockMatching()
        for lvl in range(len(c["block"])):
            got = mf.stage_get_mvs(lvl, 2).astype(np.int32)
            bad = np.argwhere((got != finals[lvl]).any(-1))
            assert bad.size == 0, "run %d level %d: %d final 2x2 cells differ, first at %s: oracle %s gpu %s" % (
                run, lvl, len(bad), bad[0], finals[lvl][tuple(bad[0])], got[tuple(bad[0])])
        assert np.array_equal(flow, oflow), "run %d" % run
    mf.close()


@pytest.mark.parametrize("env", [{}, {"BBME_SEARCH_SPLIT_BLOCKS": "0"}, {"BBME_GENERIC_SEARCH": "1"}], ids=_env_id)
def test_batched_context_mixes_the_families(bbme, oracle, env):
    """Four pairs behind one launch sequence, one family each (the pair is the kernels' second grid dimension): whole frames on
    one level, where the level-0 planes are the frames themselves."""
    c = H.LIMIT_CONTENTS[H.LIMIT_BATCH_CONTENTS[0]]
    pairs, exp = [], []
    for name in H.LIMIT_BATCH_CONTENTS:
        (p1,), (p2,), (_, oflow, _) = expected_stages(oracle, name)
        pairs.append((p1, p2))
        exp.append(oflow)
    with knobs(env):
        mb = bbme.MFBatch(pairs, c["search"], c["block"], 1)
    assert (mb.padded_height, mb.padded_width) == pairs[0][0].shape
    for spec in (True, False):
        mb.set_speculation(spec)
        got = mb.calcMotionBlockMatching()
        for p, name in enumerate(H.LIMIT_BATCH_CONTENTS):
            assert np.array_equal(got[p], exp[p]), "pair %d (%s), speculation %s: %d values differ" % (
                p, name, spec, int((got[p] != exp[p]).sum()))
    mb.close()


# ---- 3. energies beyond 2^24 and vectors at their bounds --------------------------------------------------------------------
# (not with a solver of ONE wave in all: it takes 24 s over the 262 144 blocks of the b = 2 grid, of which 97 % change)
ENERGY_FORMS = dict({"default": {}}, **{k: v for k, v in H.LIMIT_REG_FORMS.items() if k != "solve_one_wave"})


@pytest.mark.parametrize("form", list(ENERGY_FORMS))
@pytest.mark.parametrize("kind", H.ENERGY_FIELDS)
@pytest.mark.parametrize("b", H.ENERGY_BLOCKS)
def test_energies_beyond_2_pow_24(bbme, oracle, b, kind, form):
    """float32 energies SAD + (lambda * mult) * S that are rounded, not exact: the winner must still be the reference's, because
    the expression and its order are the reference's.  No tolerance.  "random": large random vectors; "ties": neighbourhoods in
    which two candidates have equal S, so that the rounding of the sum decides between them."""
    g = H.ENERGY_LEVEL
    B = g["block"][0]
    key = ("energy", b, kind)
    if key not in _expected:
        p1, p2, field = H.energy_case(b, kind)
        omf = oracle.OracleMF(search_size=g["search"], block_size=g["block"], planes1=p1, planes2=p2)
        _expected[key] = (p1, p2, field, [H.oracle_sweeps_from_grid(oracle, omf, 0, B, b, field, m) for m in H.ENERGY_RUNS])
        omf.close()
    p1, p2, field, exp = _expected[key]
    with knobs(ENERGY_FORMS[form]):
        mf = H.make_mf_from_planes(bbme, p1, p2, g["search"], g["block"])
    for mults, want in zip(H.ENERGY_RUNS, exp):
        mf.stage_set_mvs(0, b, field)
        for mult, e in zip(mults, want):
            mf.stage_regularize(0, b, mult)
            got = mf.stage_get_mvs(0, b).astype(np.int32)
            bad = np.argwhere((got != e).any(-1))
            assert bad.size == 0, "b=%d %s %s run %s sweep %d: %d of %d blocks differ, first at %s: oracle %s gpu %s" % (
                b, kind, form, mults, mult, len(bad), e.shape[0] * e.shape[1], bad[0], e[tuple(bad[0])], got[tuple(bad[0])])
    mf.close()


@pytest.mark.parametrize("forward", ["0", "1"])
@pytest.mark.parametrize("name", list(H.GUARD_CASES))
def test_memo_guard_at_8192(bbme, oracle, name, forward):
    """The memo packs a vector into 2 x 14 bits.  On a level of 8192 it serves vectors of up to +-8176 (looked up, and right); on
    a level of 8448 the host must switch it off (never looked up) and the grids must still be the oracle's."""
    w, h, memo_allowed = H.GUARD_CASES[name]
    b = H.GUARD_BLOCK
    p1, p2, field = H.guard_case(name)
    omf = oracle.OracleMF(search_size=[H.GUARD_SEARCH], block_size=[b], planes1=p1, planes2=p2)
    exp = H.oracle_sweeps_from_grid(oracle, omf, 0, b, b, field)
    omf.close()
    with knobs({"BBME_MEMO": "1", "BBME_MEMO_FORWARD": forward}):
        mf = H.make_mf_from_planes(bbme, p1, p2, [H.GUARD_SEARCH], [b])
    mf.stage_set_mvs(0, b, field)
    lookups = 0
    for mult, e in zip((1, 2), exp):
        mf.stage_regularize(0, b, mult)
        got = mf.stage_get_mvs(0, b).astype(np.int32)
        lookups += mf.sweep_stats()[9]
        bad = np.argwhere((got != e).any(-1))
        assert bad.size == 0, "%s sweep %d: %d blocks differ, first at %s: oracle %s gpu %s" % (
            name, mult, len(bad), bad[0], e[tuple(bad[0])], got[tuple(bad[0])])
    mf.close()
    print("%s forward=%s: memo lookups %d" % (name, forward, lookups))
    if memo_allowed:
        assert lookups > 0, "the memo was not used on a level it is allowed on"
    else:
        assert lookups == 0, "the memo ran on a level whose vectors its 14-bit packing cannot hold"


@pytest.mark.parametrize("env", [{}, {"BBME_MEMO": "1", "BBME_MEMO_MIN_B": "8", "BBME_MEMO_FORWARD": "1"},
                                 {"BBME_PASS1_STRIP": "1", "BBME_PASS1_LANES_MAX": "0"}, {"BBME_GENERIC_SEARCH": "1"},
                                 {"BBME_SEARCH_SPLIT_BLOCKS": "100000000"}], ids=_env_id)
def test_vectors_at_the_bounds_of_int16(bbme, oracle, env):
    """Grids holding +-32767, +-16384 and (-32768, -32768), the value the memo uses for "never a motion vector".  In the sweeps such
    candidates are outside the plane and score FLT_MAX.  The finer level's search doubles them as copyMVs does (in float there,
    in int here: +-65534 and +-32768 are exact in both), finds the predicted block outside the plane and stores a zero vector
    (:304-310): the contract is the oracle's result, and no vector may wrap."""
    g = H.INT16_LEVELS
    B0, B1 = g["block"]
    for b in (16, 8, 2):
        p1, p2, field = H.int16_case(b)
        omf = oracle.OracleMF(search_size=g["search"], block_size=g["block"], planes1=p1, planes2=p2)
        with knobs(env):
            mf = H.make_mf_from_planes(bbme, p1, p2, g["search"], g["block"])
        exp = H.oracle_sweeps_from_grid(oracle, omf, 1, B1, b, field)
        mf.stage_set_mvs(1, b, field)
        for mult, e in zip((1, 2), exp):
            mf.stage_regularize(1, b, mult)
            got = mf.stage_get_mvs(1, b).astype(np.int32)
            bad = np.argwhere((got != e).any(-1))
            assert bad.size == 0, "level 1 b=%d sweep %d: %d blocks differ, first at %s: oracle %s gpu %s" % (
                b, mult, len(bad), bad[0], e[tuple(bad[0])], got[tuple(bad[0])])
        if b == 2:
            # search_prediction straight from the injected grid, then from the grid the sweeps left
            for grid in (field, exp[1].astype(np.int16)):
                want = H.oracle_search_from_coarse(omf, grid, B1, B0)
                mf.stage_set_mvs(1, 2, grid)
                mf.stage_search(0)
                got = mf.stage_get_mvs(0, B0).astype(np.int32)
                bad = np.argwhere((got != want).any(-1))
                assert bad.size == 0, "level 0 search: %d blocks differ, first at %s: oracle %s gpu %s" % (
                    len(bad), bad[0], want[tuple(bad[0])], got[tuple(bad[0])])
        mf.close()
        omf.close()


# ---- 4. the two reductions --------------------------------------------------------------------------------------------------
def _saturated_stats(stats, pixels, what):
    assert stats["pixels"] == pixels and stats["skipped"] == 0, (what, stats)
    assert stats["sse"] == 65025 * pixels, (what, stats["sse"], 65025 * pixels)
    assert stats["sad"] == 255 * pixels, (what, stats["sad"], 255 * pixels)


@pytest.mark.parametrize("flip", [False, True], ids=["dark_on_bright", "bright_on_dark"])
def test_compensation_statistics_at_saturation(bbme, flip):
    """k_motion_compensate's sums with every pixel at the largest residual: image1 = 0, image2 = 255 (and the mirror) under a zero
    field, at a 4K level 0: SSE = 65 025 * pixels (beyond 2^32) and SAD = 255 * pixels, exactly."""
    w, h = 3840, 2160
    f1, f2 = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    if flip:
        f1, f2 = f2, f1
    window = (37, 21, 3001, 1999)
    mf = bbme.MF(f1, f2, [20], [16], 1)
    assert (mf.padded_height, mf.padded_width) == (h, w)
    assert not mf.calcMotionBlockMatching().any()             # all candidates tie: the zero vector (tests/test_limits_cpu.py)
    for block in (1, 2, 16):
        _saturated_stats(mf.compensation_error(0, block), w * h, "block %d, whole plane" % block)
        _saturated_stats(mf.compensation_error(0, block, window), window[2] * window[3], "block %d, window" % block)
        assert np.array_equal(mf.draw_MVimage(0, block), f2)
    mf.close()
    mb = bbme.MFBatch([(f1, f2), (f2, f1), (f1, f2)], [20], [16], 1)
    for flow in mb.calcMotionBlockMatching():
        assert not flow.any()
    for block in (1, 2, 16):
        for win, pixels in ((None, w * h), (window, window[2] * window[3])):
            stats = mb.compensation_errors(0, block, win)
            assert len(stats) == 3
            for p, s in enumerate(stats):
                _saturated_stats(s, pixels, "pair %d block %d window %s" % (p, block, win))
    mb.close()


@pytest.fixture(scope="module")
def epe_context(bbme):
    f1, f2, _ = bbme.synth_pair(648, 488, 4711, max_motion=12)
    mf = bbme.MF(f1, f2, [24, 24], [8, 8], 2)
    mf.calcMotionBlockMatching()
    cells = mf.get_cells()
    assert len({tuple(v) for v in cells.reshape(-1, 2).tolist()}) > 20          # a field with many different vectors
    yield mf, cells
    mf.close()


@pytest.mark.parametrize("kind", ["plain", "holes", "unknown"])
@pytest.mark.parametrize("scale", [1, 3])
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_epe_reduction_shapes_and_unknowns(bbme, epe_context, size, scale, kind):
    """k_epe with a ground truth smaller than one workgroup (5 x 3) and one of more than 512 * 256 pixels (several trips of the
    grid-stride loop; at scale 3 the largest that fits the frame), at scales 1 and 3, with +-inf, NaN and values just below, at
    and above 1e9, and with nothing known (NaN, as include/bbme.h says).  Reference: float64 sum in numpy of the float32
    per-pixel expression; tolerance: the rel = 1e-12 the header states for another order of the sum."""
    import torch
    mf, cells = epe_context
    if size == "tiny":
        gh, gw = 3, 5
    else:
        gh, gw = -(-mf.orig_height // scale), -(-mf.orig_width // scale)
        assert scale != 1 or gh * gw > 512 * 256
    gt = H.epe_ground_truth(gh, gw, kind, np.random.default_rng(gh * 7 + scale))
    want = H.epe_reference(gt, cells, mf.padding_x, mf.padding_y, scale)
    got = mf.calculate_mse_device(torch.from_numpy(gt).cuda(), scale=scale)
    print("epe %s scale %d %s: gpu %r reference %r" % (size, scale, kind, got, want))
    if kind == "unknown":
        assert np.isnan(want) and np.isnan(got)
    else:
        assert np.isfinite(want) and got == pytest.approx(want, rel=1e-12)
