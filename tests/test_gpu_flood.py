"""Flood speculation in the solver's chain rounds (k_reg_solve<.., true>, BBME_FLOOD_RULE; csrc/bbme_kernels.hpp).  A kept speculative
evaluation is an ordinary owned evaluation, so whatever the rule selects and whatever the waves make of it the field must stay the
CPU oracle's, bit for bit.  The default rule takes the variant to grids of >= 100 000 blocks at b >= 8, which no test shape has: the
rule is forced onto every sweep at every block size ("2,0"), at depth 1 and at the default depth, and combined with the settings
that change what a round finds in its queue -- one workgroup per XCD (every round hands blocks over, mailboxes at their cap),
single-wave workgroups (no siblings), the hand-over off -- with eager launches, and with the speculative search on every level
and off.  One case reads the new counter (bbme_sweep_stats [15]): speculative evaluations were made AND kept, so the suite cannot
pass without reaching the code."""
import functools
import os

import numpy as np
import pytest

from helpers import gpu_schedule, oracle_schedule

pytestmark = pytest.mark.gpu

# (width, height, levels): the issue's two shapes; block sizes 16 and 8, so that sweeps at 8 x 8 exist at both.  Seed 20 with 2 x 2
# motion tiles is the pair of tests/test_flood_model_cpu.py (a 32-round chain at level 0, b = 8)
SHAPES = {"512x384": (512, 384, 3), "256x192": (256, 192, 2)}
BLOCKS = {16: 48, 8: 40}                        # block size: search size
SEEDS = (20, 21)                                # the second pair of a batch
FORCED = "2,0"                                  # every sweep, default depth
SETTINGS = {
    "default_rule": {},
    "forced": {"BBME_FLOOD_RULE": FORCED},
    "forced_depth1": {"BBME_FLOOD_RULE": FORCED + ",1"},
    "forced_depth3": {"BBME_FLOOD_RULE": FORCED + ",3"},
    "one_wg_per_xcd": {"BBME_FLOOD_RULE": FORCED, "BBME_SOLVE_WGS": "8", "BBME_WIDE_THRESHOLD": "100000"},
    "one_wg_per_xcd_depth1": {"BBME_FLOOD_RULE": FORCED + ",1", "BBME_SOLVE_WGS": "8", "BBME_WIDE_THRESHOLD": "100000"},
    "single_wave": {"BBME_FLOOD_RULE": FORCED, "BBME_SOLVE_WAVES": "1"},
    "no_handover": {"BBME_FLOOD_RULE": FORCED, "BBME_SOLVE_SHARE": "0"},
    "eager": {"BBME_FLOOD_RULE": FORCED, "BBME_NO_GRAPH": "1"},
    "search_speculated": {"BBME_FLOOD_RULE": FORCED, "BBME_SPEC_MIN_GABS": "0"},
    "search_in_line": {"BBME_FLOOD_RULE": FORCED, "BBME_SPECULATE": "0"},
}


def _pair(bbme, shape, seed=SEEDS[0]):
    w, h, _ = SHAPES[shape]
    return bbme.synth_pair(w, h, seed, max_motion=20, tiles=2)[:2]


def _geometry(shape, block):
    levels = SHAPES[shape][2]
    return [BLOCKS[block]] * levels, [block] * levels


@functools.lru_cache(maxsize=None)
def _expected(bbme, oracle, shape, block, seed=SEEDS[0]):
    f1, f2 = _pair(bbme, shape, seed)
    search, blocks = _geometry(shape, block)
    omf = oracle.OracleMF(f1, f2, search, blocks)
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


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("block", list(BLOCKS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_field_against_the_oracle(bbme, oracle, shape, block, setting):
    f1, f2 = _pair(bbme, shape)
    search, blocks = _geometry(shape, block)
    exp = _expected(bbme, oracle, shape, block)
    mf = _create(SETTINGS[setting], lambda: bbme.MF(f1, f2, search, blocks, len(blocks)))
    for run in ("first", "second"):
        assert np.array_equal(mf.calcMotionBlockMatching(), exp), "%s, B = %d, %s, %s estimate" % (shape, block, setting, run)
    mf.close()


@pytest.mark.parametrize("setting", ["forced", "forced_depth1", "one_wg_per_xcd", "search_in_line"])
@pytest.mark.parametrize("block", list(BLOCKS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_of_two_pair_by_pair(bbme, oracle, shape, block, setting):
    pairs = [_pair(bbme, shape, seed) for seed in SEEDS]
    search, blocks = _geometry(shape, block)
    mb = _create(SETTINGS[setting], lambda: bbme.MFBatch(pairs, search, blocks, len(blocks)))
    got = [mb.calcMotionBlockMatching() for _ in range(2)]
    mb.close()
    for p, seed in enumerate(SEEDS):
        exp = _expected(bbme, oracle, shape, block, seed)
        for run in range(2):
            assert np.array_equal(got[run][p], exp), "%s, B = %d, %s: pair %d, estimate %d" % (shape, block, setting, p, run)


@pytest.mark.parametrize("depth", (1, 2))
def test_speculative_evaluations_are_kept(bbme, oracle, depth):
    """Stage by stage at 512 x 384, B = 16, every grid against the oracle's; the rule forced on: over the pyramid, and in the sweeps at
    8 x 8 alone, evaluations made on speculation counted.  At depth 0 the rule selects nothing and the counter stays 0: the plain solver never writes it."""
    f1, f2 = _pair(bbme, "512x384")
    search, blocks = _geometry("512x384", 16)
    L = len(blocks)
    omf = oracle.OracleMF(f1, f2, search, blocks)
    exp = []
    oracle_schedule(omf, L, lambda *a: exp.append(a))
    omf.close()
    for env, forced in (({"BBME_FLOOD_RULE": "%s,%d" % (FORCED, depth)}, True), ({"BBME_FLOOD_RULE": FORCED + ",0"}, False)):
        mf = _create(env, lambda: bbme.MF(f1, f2, search, blocks, L))
        kept = {}

        def on_stage(name, lvl, b, mvs):
            en, el, eb, ev = exp[on_stage.i]
            on_stage.i += 1
            assert (en, el, eb) == (name, lvl, b) and np.array_equal(ev, mvs), "stage %s level %d block %d" % (name, lvl, b)
            if name != "search":
                kept[(lvl, b, name)] = mf.sweep_stats()[15]
        on_stage.i = 0
        gpu_schedule(mf, L, blocks, on_stage)
        mf.close()
        print("BBME_FLOOD_RULE %s: kept per sweep %s" % (env.get("BBME_FLOOD_RULE"), kept))
        if forced:
            assert sum(kept.values()) > 0, kept
            assert sum(v for (lvl, b, name), v in kept.items() if b == 8) > 0, kept
        else:
            assert not any(kept.values()), kept
