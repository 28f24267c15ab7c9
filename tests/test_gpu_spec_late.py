"""The speculative search's late predictions (newest_coarse_grid, csrc/bbme_kernels.hpp): a block of the search that runs beside
the coarser level's late sweeps takes its prediction from the newest grid of that level that is complete when the block starts.
Whatever it reads, the fix-up behind the search compares the recorded vector with the final one, so the field must stay the CPU
oracle's, bit for bit, with BBME_SPEC_LATE = 0 (every block predicts from the grid at the fork), 1 (the default) and 2 (test
setting: every block reads the LAST grid of the table, which at that moment is unwritten, half written or holds a grid of another
geometry).  The speculation is forced onto every level, every context estimates twice (the second replay starts with the first
one's final count still in the published word), and bbme_fixup_counts must report, at 0, exactly the blocks whose prediction
differs between the oracle's grid after the two sweeps at B and its final grid."""
import functools
import os

import numpy as np
import pytest

from helpers import oracle_schedule

pytestmark = pytest.mark.gpu

# name: (width, height, seed, max_motion, search sizes, block sizes) -- the smallest shapes at which each clause can fail:
#   b16: late sweeps at 8, 4 and 2, so big[] holds three grid geometries in turn;  b8: the coarse level leaves only 4 and 2;
#   mixed: the reference's second literal set, the coarse block differs per level;
#   outside: motion at the search range, predictions that leave the image
CASES = {
    "b16": (512, 384, 3101, 20, [48, 48, 48], [16, 16, 16]),
    "b8": (512, 384, 3101, 20, [40, 40, 40], [8, 8, 8]),
    "mixed": (584, 388, 3102, 10, [32, 32, 42], [16, 16, 32]),
    "outside": (256, 192, 3103, 16, [48, 48, 48], [16, 16, 16]),
}
BATCH_SEEDS = (3101, 3111, 3121)          # pairs of the "b16" shape; the first one is the case itself
LATE = (0, 1, 2)


def _pair(bbme, name, seed=None):
    w, h, case_seed, mm, search, block = CASES[name]
    f1, f2, _ = bbme.synth_pair(w, h, case_seed if seed is None else seed, max_motion=mm)
    return f1, f2, search, block


@functools.lru_cache(maxsize=None)
def _expected(bbme, oracle, name, seed=None):
    """The oracle's field, and per level the blocks whose prediction differs between the coarser level's grid after its two
    sweeps at its own block size and its final grid of 2 x 2 cells (copyMVs reads the top-left cell of the coarse block)."""
    f1, f2, search, block = _pair(bbme, name, seed)
    L = len(block)
    omf = oracle.OracleMF(f1, f2, search, block)
    grids = {}
    flow = oracle_schedule(omf, L, lambda kind, lvl, b, mv: grids.__setitem__((kind, lvl, b), mv))
    listed, blocks = [0] * L, [0] * L
    for lvl in range(L):
        h, w = omf.level_shape(lvl)
        blocks[lvl] = (h // block[lvl]) * (w // block[lvl])
        if lvl == L - 1:
            continue
        B1 = block[lvl + 1]
        ci = (np.arange(0, h, block[lvl]) // (2 * B1)) * B1
        cj = (np.arange(0, w, block[lvl]) // (2 * B1)) * B1
        at_fork = grids[("sweep2", lvl + 1, B1)][(ci // B1)[:, None], (cj // B1)[None, :]]
        final = grids[("sweep2", lvl + 1, 2)][(ci // 2)[:, None], (cj // 2)[None, :]]
        listed[lvl] = int((at_fork != final).any(-1).sum())
    omf.close()
    flow.setflags(write=False)
    return flow, tuple(listed), tuple(blocks)


def _create(late, make, **more):
    """make() with the speculation forced onto every level and BBME_SPEC_LATE = late (knobs are read at context creation)."""
    env = {"BBME_SPEC_MIN_GABS": "0", "BBME_SPEC_LATE": str(late), **more}
    os.environ.update(env)
    try:
        return make()
    finally:
        for key in env:
            del os.environ[key]


def _check_counts(counts, late, listed, blocks, what):
    print("%s BBME_SPEC_LATE=%d: listed %s, at the fork %s, blocks %s" % (what, late, counts, list(listed), list(blocks)))
    assert counts[-1] == 0, "%s: the coarsest level is never speculated" % what
    if late == 0:
        assert counts == list(listed), what
    else:
        assert all(0 <= c <= n for c, n in zip(counts, blocks)), what


@pytest.mark.parametrize("late", LATE)
@pytest.mark.parametrize("name", list(CASES))
def test_field_and_fixup_counts_against_the_oracle(bbme, oracle, name, late):
    f1, f2, search, block = _pair(bbme, name)
    exp, listed, blocks = _expected(bbme, oracle, name)
    if name == "outside":
        assert any(listed), "no prediction changes behind the fork: the case checks nothing"
    mf = _create(late, lambda: bbme.MF(f1, f2, search, block, len(block)))
    for run in ("first", "second"):
        got = mf.calcMotionBlockMatching()
        assert np.array_equal(got, exp), "%s, BBME_SPEC_LATE=%d, %s estimate" % (name, late, run)
        _check_counts(mf.fixup_counts(), late, listed, blocks, "%s, %s estimate" % (name, run))
    mf.close()


@pytest.mark.parametrize("late", LATE)
def test_batched_context_pair_by_pair(bbme, oracle, late):
    """Three pairs behind one launch sequence: a published word, a fix-up counter and grid strides per pair.  Every pair against
    a context of its own (and that one against the oracle)."""
    pairs = [_pair(bbme, "b16", seed)[:2] for seed in BATCH_SEEDS]
    _, _, search, block = _pair(bbme, "b16")
    mb = _create(late, lambda: bbme.MFBatch(pairs, search, block, len(block)))
    got = [mb.calcMotionBlockMatching() for _ in range(2)]
    counts = [mb.fixup_counts(p) for p in range(len(pairs))]
    mb.close()
    for p, seed in enumerate(BATCH_SEEDS):
        exp, listed, blocks = _expected(bbme, oracle, "b16", seed)
        own = _create(late, lambda: bbme.MF(pairs[p][0], pairs[p][1], search, block, len(block)))
        own_flow = [own.calcMotionBlockMatching() for _ in range(2)]
        own_counts = own.fixup_counts()
        own.close()
        for run in range(2):
            assert np.array_equal(own_flow[run], exp), "pair %d alone, estimate %d" % (p, run)
            assert np.array_equal(got[run][p], own_flow[run]), "pair %d of the batch, estimate %d" % (p, run)
        _check_counts(counts[p], late, listed, blocks, "pair %d of the batch" % p)
        _check_counts(own_counts, late, listed, blocks, "pair %d alone" % p)


@pytest.mark.parametrize("late", (1, 2))
@pytest.mark.parametrize("fork_first", (0, 1))
@pytest.mark.parametrize("name", ["b16", "mixed"])
def test_either_fork_point(bbme, oracle, name, fork_first, late):
    """The search forked behind the first sweep at B (the default: the table starts one grid earlier, the published count with it)
    and behind the second (BBME_SPEC_FORK_FIRST=0): same field, counts within the level."""
    f1, f2, search, block = _pair(bbme, name)
    exp, listed, blocks = _expected(bbme, oracle, name)
    mf = _create(late, lambda: bbme.MF(f1, f2, search, block, len(block)), BBME_SPEC_FORK_FIRST=str(fork_first))
    for run in ("first", "second"):
        assert np.array_equal(mf.calcMotionBlockMatching(), exp), "%s, fork_first %d, BBME_SPEC_LATE=%d, %s estimate" % (name, fork_first, late, run)
        _check_counts(mf.fixup_counts(), late, listed, blocks, "%s, fork_first %d, %s estimate" % (name, fork_first, run))
    mf.close()


def test_fixup_counts_without_speculation(bbme):
    """Levels whose search is not speculative report 0: below the default threshold, and with the speculation switched off."""
    f1, f2, search, block = _pair(bbme, "outside")
    mf = bbme.MF(f1, f2, search, block, len(block))
    mf.calcMotionBlockMatching()
    assert mf.fixup_counts() == [0, 0, 0]
    mf.close()
    mf = _create(1, lambda: bbme.MF(f1, f2, search, block, len(block)))
    mf.calcMotionBlockMatching()
    with pytest.raises(bbme.BbmeError):
        mf.fixup_counts(1)                       # a single context has one pair
    mf.set_speculation(False)
    mf.calcMotionBlockMatching()
    assert mf.fixup_counts() == [0, 0, 0]
    mf.close()
