"""Pass 1's head (k_reg_pass1, k_reg_pass1_lanes, k_reg_pass1_strip; csrc/bbme_kernels.hpp, "PASS 1'S HEAD").  The three kernels
index threads, blocks, rows and columns in 32 bits, divide by the grid's width once, address the old grid, the estimates, the
flag map and the image rows at 32-bit byte offsets from the pair's base, shift only the pointers they read from pair to pair and
compare the result with candidate 0 of the evaluation instead of loading the block's old value again.  None of that may change
a value: every case compares the cells (get_cells) with the CPU oracle's, bit for bit -- the full field, and the Jacobi mode,
which is pass 1 alone and so shows these kernels' output directly -- on

  100 x 52, block 4, one level      grids of 25 x 13 (b = 4) and 50 x 26 (b = 2): odd columns, columns that are no multiple of 4,
                                    block counts that are no multiple of a workgroup's
  72 x 40, block 8, three levels    the coarsest grid is three blocks wide
  352 x 256, block 16, three levels as a single context and as a batch of two (the pair's shift, blockIdx.y = 1)
  1024 x 576, search 24, blocks 8   147 456 blocks at 2 x 2: the one geometry at which a single pair reaches the large-grid and
                                    strip forms by itself

with each form of pass 1 forced through its knobs -- the defaults, the b-lanes form on every grid, the strip form eager and lazy
-- replayed from a graph and launched eagerly."""
import functools
import os

import numpy as np
import pytest

from helpers import oracle_schedule

pytestmark = pytest.mark.gpu

# name: (width, height, search, block, seed, max motion)
SHAPES = {
    "100x52": (100, 52, [12], [4], 3101, 3),
    "72x40": (72, 40, [24] * 3, [8] * 3, 3102, 4),
    "352x256": (352, 256, [48] * 3, [16] * 3, 3103, 20),
    "1024x576": (1024, 576, [24, 24], [8, 8], 3104, 8),
}
BATCH_SEED = 3105                               # the second pair of the batch of two
FORMS = {
    "defaults": {},
    "lanes_max_0": {"BBME_PASS1_LANES_MAX": "0"},
    "strip_eager": {"BBME_PASS1_STRIP": "1", "BBME_PASS1_LAZY": "0"},
    "strip_lazy": {"BBME_PASS1_STRIP": "1", "BBME_PASS1_LAZY": "1", "BBME_RELAX_STEPS": "1"},
}
LAUNCH = {"graph": {}, "no_graph": {"BBME_NO_GRAPH": "1"}}


def _pair(bbme, name, seed=None):
    w, h, _, _, s, mm = SHAPES[name]
    return bbme.synth_pair(w, h, s if seed is None else seed, max_motion=mm, tiles=2)[:2]


@functools.lru_cache(maxsize=None)
def _expected(bbme, oracle, name, seed, jacobi):
    """The oracle's cells (CH, CW, 2) int16 of the whole schedule; computed once per (shape, pair, mode), read-only."""
    _, _, search, block, _, _ = SHAPES[name]
    f1, f2 = _pair(bbme, name, seed)
    omf = oracle.OracleMF(f1, f2, search, block)
    omf.set_jacobi_regularizer(jacobi)
    oracle_schedule(omf, len(block))
    cells = omf.block_mvs(0, 2).astype(np.int16)
    omf.close()
    cells.setflags(write=False)
    return cells


def _create(env, make):
    before = {key: os.environ.get(key) for key in env}
    os.environ.update(env)                      # knobs are read at context creation
    try:
        return make()
    finally:
        for key, value in before.items():
            if value is None:
                del os.environ[key]
            else:
                os.environ[key] = value


@pytest.mark.parametrize("launch", list(LAUNCH))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("jacobi", [False, True], ids=["full", "jacobi"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_cells_against_the_oracle(bbme, oracle, name, jacobi, form, launch):
    _, _, search, block, seed, _ = SHAPES[name]
    f1, f2 = _pair(bbme, name)
    exp = _expected(bbme, oracle, name, seed, jacobi)
    mf = _create(dict(FORMS[form], **LAUNCH[launch]), lambda: bbme.MF(f1, f2, search, block, len(block)))
    try:
        if jacobi:
            mf.set_regularizer_mode(True)
        for run in ("first", "second"):
            mf.estimate_async()
            got = mf.get_cells()
            assert np.array_equal(got, exp), "%s, %s, %s, %s estimate: %d of %d cells differ" % (
                name, form, launch, run, int((got != exp).any(axis=2).sum()), exp.shape[0] * exp.shape[1])
    finally:
        mf.close()


@pytest.mark.parametrize("launch", list(LAUNCH))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("jacobi", [False, True], ids=["full", "jacobi"])
def test_batch_of_two_pair_by_pair(bbme, oracle, jacobi, form, launch):
    name = "352x256"
    _, _, search, block, seed, _ = SHAPES[name]
    seeds = (seed, BATCH_SEED)
    pairs = [_pair(bbme, name, s) for s in seeds]
    mb = _create(dict(FORMS[form], **LAUNCH[launch]), lambda: bbme.MFBatch(pairs, search, block, len(block)))
    try:
        if jacobi:
            mb.set_regularizer_mode(True)
        for run in ("first", "second"):
            mb.estimate_async()
            for p, s in enumerate(seeds):
                assert np.array_equal(mb.get_pair_cells(p), _expected(bbme, oracle, name, s, jacobi)), \
                    "%s, %s: pair %d, %s estimate" % (form, launch, p, run)
    finally:
        mb.close()
