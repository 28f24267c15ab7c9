"""The solver's rounds and its launch head (k_reg_solve; csrc/bbme_kernels.hpp, "HOT AND COLD ARGUMENTS").  The kernel keeps in
registers only what a round reads and fetches the rest -- overflow lists, counters, the publish word, the statistics switch --
from its kernel-argument segment where it is used; the first scan step's flags are asked for ahead of the set-up; a speculating
round asks for its candidates before it works out its links.  None of that may change a value: every case compares the field with
the CPU oracle's, bit for bit, on the shapes of tests/test_gpu_flood.py, under the default rule and with the flood variant forced
onto every sweep, and under the settings that change what a launch finds: one workgroup per XCD (every queue overflows into the
mailboxes), single-wave workgroups, the hand-over off, eager launches, the speculative search on every level.  Further: a 72 x 40
pair at b = 8 (45 blocks: the flag map ends inside a 16-flag segment) with one level and with three (the coarsest grid is then three
blocks wide: the flood depth falls to 0); a batch of two pairs (the pair's shift of every hot base); R = 127 at B = 16 (the
largest image offsets a test shape reaches); and one case that reads bbme_sweep_stats [15], which now is fetched by the epilogue."""
import functools
import os

import numpy as np
import pytest

from helpers import gpu_schedule, oracle_schedule

pytestmark = pytest.mark.gpu

SHAPES = {"512x384": (512, 384, 3), "256x192": (256, 192, 2)}        # (width, height, levels)
BLOCKS = {16: 48, 8: 40}                        # block size: search size
SEEDS = (20, 21)
FORCED = "2,0"                                  # the flood variant in every sweep, default depth
ONE_WG = {"BBME_SOLVE_WGS": "8", "BBME_WIDE_THRESHOLD": "100000"}
SETTINGS = {
    "default": {},
    "forced": {"BBME_FLOOD_RULE": FORCED},
    "forced_one_wg_per_xcd": dict(ONE_WG, BBME_FLOOD_RULE=FORCED),
    "single_wave": {"BBME_SOLVE_WAVES": "1"},
    "no_handover": {"BBME_SOLVE_SHARE": "0"},
    "eager": {"BBME_NO_GRAPH": "1"},
    "search_speculated": {"BBME_SPEC_MIN_GABS": "0"},
    "forced_single_wave": {"BBME_FLOOD_RULE": FORCED, "BBME_SOLVE_WAVES": "1"},
    "forced_no_handover": {"BBME_FLOOD_RULE": FORCED, "BBME_SOLVE_SHARE": "0"},
    "forced_eager": {"BBME_FLOOD_RULE": FORCED, "BBME_NO_GRAPH": "1"},
    "forced_search_speculated": {"BBME_FLOOD_RULE": FORCED, "BBME_SPEC_MIN_GABS": "0"},
}


def _pair(bbme, width, height, seed):
    return bbme.synth_pair(width, height, seed, max_motion=20, tiles=2)[:2]


@functools.lru_cache(maxsize=None)
def _expected(bbme, oracle, width, height, seed, search, blocks):
    f1, f2 = _pair(bbme, width, height, seed)
    omf = oracle.OracleMF(f1, f2, list(search), list(blocks))
    flow = omf.calc_motion_block_matching().copy()
    omf.close()
    flow.setflags(write=False)
    return flow


def _create(env, make):
    before = {key: os.environ.get(key) for key in env}
    os.environ.update(env)                      # knobs are read at context creation
    try:
        return make()
    finally:
        for key, value in before.items():       # (a rule forced onto the whole suite from outside stays)
            if value is None:
                del os.environ[key]
            else:
                os.environ[key] = value


def _check(bbme, oracle, width, height, search, blocks, setting, what):
    f1, f2 = _pair(bbme, width, height, SEEDS[0])
    exp = _expected(bbme, oracle, width, height, SEEDS[0], tuple(search), tuple(blocks))
    mf = _create(SETTINGS[setting], lambda: bbme.MF(f1, f2, search, blocks, len(blocks)))
    try:
        for run in ("first", "second"):
            assert np.array_equal(mf.calcMotionBlockMatching(), exp), "%s, %s, %s estimate" % (what, setting, run)
    finally:
        mf.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("block", list(BLOCKS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_field_against_the_oracle(bbme, oracle, shape, block, setting):
    w, h, levels = SHAPES[shape]
    _check(bbme, oracle, w, h, [BLOCKS[block]] * levels, [block] * levels, setting, "%s, B = %d" % (shape, block))


@pytest.mark.parametrize("setting", ["default", "forced", "forced_one_wg_per_xcd", "forced_single_wave"])
@pytest.mark.parametrize("levels", (1, 3))
def test_small_grid_with_a_ragged_flag_map(bbme, oracle, levels, setting):
    """72 x 40 at b = 8: 9 x 5 = 45 blocks, so the last flag segment is part padding; with three levels the coarsest grid is three
    blocks wide and a flood has no direction to follow."""
    _check(bbme, oracle, 72, 40, [24] * levels, [8] * levels, setting, "72x40, %d level(s)" % levels)


@pytest.mark.parametrize("setting", ["default", "forced", "forced_one_wg_per_xcd"])
def test_largest_range(bbme, oracle, setting):
    """R = 127 at B = 16 on 256 x 192: the padded planes are the widest a test shape has, the image offsets the largest."""
    _check(bbme, oracle, 256, 192, [16 + 2 * 127], [16], setting, "256x192, R = 127")


@pytest.mark.parametrize("setting", ["default", "forced", "forced_one_wg_per_xcd", "forced_no_handover"])
@pytest.mark.parametrize("block", list(BLOCKS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_of_two_pair_by_pair(bbme, oracle, shape, block, setting):
    w, h, levels = SHAPES[shape]
    search, blocks = [BLOCKS[block]] * levels, [block] * levels
    pairs = [_pair(bbme, w, h, seed) for seed in SEEDS]
    mb = _create(SETTINGS[setting], lambda: bbme.MFBatch(pairs, search, blocks, levels))
    try:
        got = [mb.calcMotionBlockMatching() for _ in range(2)]
    finally:
        mb.close()
    for p, seed in enumerate(SEEDS):
        exp = _expected(bbme, oracle, w, h, seed, tuple(search), tuple(blocks))
        for run in range(2):
            assert np.array_equal(got[run][p], exp), "%s, B = %d, %s: pair %d, estimate %d" % (shape, block, setting, p, run)


def test_flood_path_is_reached_and_counted(bbme, oracle):
    """Stage by stage at 512 x 384, B = 16, the rule forced on, every grid against the oracle's: bbme_sweep_stats [15] > 0 in the
    sweeps at 8 x 8 -- speculative evaluations were made and kept, and the epilogue found the statistics switch and the counters."""
    f1, f2 = _pair(bbme, 512, 384, SEEDS[0])
    search, blocks = [BLOCKS[16]] * 3, [16] * 3
    omf = oracle.OracleMF(f1, f2, search, blocks)
    exp = []
    oracle_schedule(omf, 3, lambda *a: exp.append(a))
    omf.close()
    mf = _create(SETTINGS["forced"], lambda: bbme.MF(f1, f2, search, blocks, 3))
    kept, evaluated = {}, {}

    def on_stage(name, lvl, b, mvs):
        en, el, eb, ev = exp[on_stage.i]
        on_stage.i += 1
        assert (en, el, eb) == (name, lvl, b) and np.array_equal(ev, mvs), "stage %s level %d block %d" % (name, lvl, b)
        if name != "search":
            stats = mf.sweep_stats()
            kept[(lvl, b, name)], evaluated[(lvl, b, name)] = stats[15], stats[4]
    on_stage.i = 0
    try:
        gpu_schedule(mf, 3, blocks, on_stage)
    finally:
        mf.close()
    print("kept per sweep %s\nevaluated per sweep %s" % (kept, evaluated))
    assert sum(v for (lvl, b, name), v in kept.items() if b == 8) > 0, kept
    assert sum(evaluated.values()) > 0, evaluated
