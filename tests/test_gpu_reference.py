"""The kernels against the reference's OWN compiled core, no oracle in between.  tests/golden/reference_digests.json holds
sha256 digests of what oracle/_ref/mf_ref (motion_framework.cpp compiled in place, see oracle/Makefile) computed on the cases
of tests/helpers.py (REF_*): the inputs, every stage's grid, the dense field, sweeps from injected grids, motion-compensated
frames.  Every test regenerates the inputs from their seeds, asserts the input digest first (a mismatch there is a difference
between the machines' numpy or host pyramid, not a kernel bug), runs the kernels through the C-ABI and compares digests: bit
exact, no tolerance.  tests/test_reference_core_cpu.py is the proof that the binary and the oracle agree; this file is the proof
that the kernels agree with what the binary wrote.

Nothing here needs the binary or skips.  On a mismatch, mf_ref (if it travelled with the tree) or else the oracle is run only to
name the first differing stage and block in the failure message."""
import json
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_limits import knobs

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")) as _f:
    DIGESTS = json.load(_f)

INPUT_MISMATCH = ("%s: the regenerated inputs differ from the ones the reference ran on (numpy's generators or the host "
                  "pyramid differ between the machines): not a kernel bug, regenerate tests/golden/reference_digests.json")


def explain(oracle, planes1, planes2, search, block, raster, got, what):
    """Failure message only: the first stage and block where the kernels leave the reference's (or, without the binary, the
    oracle's) grids."""
    if oracle.have_mf_ref():
        who = "mf_ref"
        exp = [(n, l, b, g.astype(np.int32)) for n, l, b, g in
               oracle.ref_stages(planes1[0], planes2[0], search, block, planes=(planes1, planes2), mode="raster" if raster else None)["stages"]]
    else:
        who = "oracle (mf_ref absent)"
        exp = H.oracle_stages_from_planes(oracle, planes1, planes2, search, block, raster)[0]
    for (n, l, b, ev), (_, _, _, gv) in zip(exp, got):
        bad = np.argwhere((ev != gv).any(-1))
        if bad.size:
            return "%s: stage %s level %d block %d: %d of %d MVs differ, first at %s: %s %s gpu %s" % (
                what, n, l, b, len(bad), ev.shape[0] * ev.shape[1], bad[0], who, ev[tuple(bad[0])], gv[tuple(bad[0])])
    return "%s: the digests differ but %s agrees with the kernels at every stage: the record is stale" % (what, who)


def input_digest(planes1, planes2, search, block):
    return H.sha256_of(np.array(list(search) + list(block), np.int32), *(list(planes1) + list(planes2)))


def run_stages(bbme, planes1, planes2, search, block, raster):
    mf = H.make_mf_from_planes(bbme, planes1, planes2, search, block, raster)
    got = []
    flow = H.gpu_schedule(mf, len(block), block, lambda n, l, b, v: got.append((n, l, b, v)))
    return mf, got, flow


def assert_stages_recorded(oracle, rec, planes1, planes2, search, block, raster, got, flow, what):
    assert [k for k, _ in rec["stages"]] == [H.stage_key(n, l, b) for n, l, b, _ in got], what
    for (key, digest), (n, l, b, v) in zip(rec["stages"], got):
        if H.sha256_of(v.astype(np.int16)) != digest:
            pytest.fail(explain(oracle, planes1, planes2, search, block, raster, got, what))
    assert H.sha256_of(flow.astype(np.float32)) == rec["flow"], "%s: the dense field differs from the reference's" % what


@pytest.mark.parametrize("name", list(H.REF_STAGE_CASES))
def test_stages_against_the_reference(bbme, oracle, name):
    """gpu_schedule stage by stage (bbme_stage_search / bbme_stage_regularize / bbme_stage_get_mvs / bbme_stage_expand)."""
    rec = DIGESTS["stages"][name]
    p1, p2, search, block, raster = H.ref_stage_case(oracle, name)
    assert input_digest(p1, p2, search, block) == rec["inputs"], INPUT_MISMATCH % name
    mf, got, flow = run_stages(bbme, p1, p2, search, block, raster)
    mf.close()
    assert_stages_recorded(oracle, rec, p1, p2, search, block, raster, got, flow, name)


@pytest.mark.parametrize("name", H.REF_SPEC_CASES)
def test_speculative_estimate_against_the_reference(bbme, oracle, name):
    """bbme_estimate whole with the speculative search and its list kernel forced onto every level (BBME_SPEC_MIN_GABS=0): the
    field and every level's final 2 x 2 grid, twice on one context."""
    rec = DIGESTS["spec"][name]
    c = H.LIMIT_CONTENTS[name]
    p1, p2 = H.limit_content_planes(name)
    assert input_digest(p1, p2, c["search"], c["block"]) == rec["inputs"], INPUT_MISMATCH % name
    finals = {key: digest for key, digest in rec["stages"]}
    with knobs({"BBME_SPEC_MIN_GABS": "0", "BBME_SPECULATE": "1"}):
        mf = H.make_mf_from_planes(bbme, p1, p2, c["search"], c["block"])
    mf.set_speculation(True)
    for run in range(2):
        flow = mf.calcMotionBlockMatching()
        for lvl in range(len(c["block"])):
            assert H.sha256_of(mf.stage_get_mvs(lvl, 2).astype(np.int16)) == finals[H.stage_key("sweep2", lvl, 2)], \
                "%s run %d: level %d's final grid differs from the reference's" % (name, run, lvl)
        assert H.sha256_of(flow.astype(np.float32)) == rec["flow"], "%s run %d: the dense field differs from the reference's" % (name, run)
    mf.close()


@pytest.mark.parametrize("seed", H.REF_RANDOM_SEEDS)
def test_random_configurations_against_the_reference(bbme, oracle, seed):
    """Ten of the random configurations, default schedule, run twice: the dense field of calcMotionBlockMatching() on an
    untouched MF of the reference."""
    rec = DIGESTS["random"][str(seed)]
    p1, p2, search, block = H.ref_random_case(oracle, seed)
    assert input_digest(p1, p2, search, block) == rec["inputs"], INPUT_MISMATCH % ("random %d" % seed)
    mf = H.make_mf_from_planes(bbme, p1, p2, search, block)
    a = mf.calcMotionBlockMatching()
    b = mf.calcMotionBlockMatching()
    mf.close()
    if H.sha256_of(a.astype(np.float32)) != rec["flow"]:
        mf, got, flow = run_stages(bbme, p1, p2, search, block, False)
        mf.close()
        pytest.fail(explain(oracle, p1, p2, search, block, False, got, "random %d %s %s" % (seed, search, block)))
    assert H.sha256_of(b.astype(np.float32)) == rec["flow"], "random %d: the second run differs from the reference" % seed


def sweep_failure(oracle, plane1, plane2, search, B, b, field, mults, got, what):
    if not oracle.have_mf_ref():
        return "%s: the grids differ from the reference's record (mf_ref absent: no block named)" % what
    for k, (e, g) in enumerate(zip(oracle.ref_sweeps(plane1, plane2, search, B, b, field, mults), got)):
        bad = np.argwhere((e.astype(np.int32) != g).any(-1))
        if bad.size:
            return "%s sweep %d: %d blocks differ, first at %s: mf_ref %s gpu %s" % (what, k, len(bad), bad[0], e[tuple(bad[0])], g[tuple(bad[0])])
    return "%s: the digests differ but mf_ref agrees with the kernels: the record is stale" % what


@pytest.mark.parametrize("form", list(H.REF_SWEEP_FORMS))
@pytest.mark.parametrize("kind", H.ENERGY_FIELDS)
@pytest.mark.parametrize("b", H.ENERGY_BLOCKS)
def test_energy_sweeps_against_the_reference(bbme, oracle, b, kind, form):
    """bbme_stage_set_mvs + sweeps where lambda * mult * S is beyond 2^24 and float32 rounding picks the winner."""
    g = H.ENERGY_LEVEL
    p1, p2, field = H.energy_case(b, kind)
    with knobs(H.REF_SWEEP_FORMS[form]):
        mf = H.make_mf_from_planes(bbme, p1, p2, g["search"], g["block"])
    for run, mults in enumerate(H.ENERGY_RUNS):
        rec = DIGESTS["sweeps"]["energy_b%d_%s_run%d" % (b, kind, run)]
        what = "energy b=%d %s %s %s" % (b, kind, mults, form)
        assert H.sha256_of(p1[0], p2[0], field) == rec["inputs"], INPUT_MISMATCH % what
        mf.stage_set_mvs(0, b, field)
        got = []
        for mult in mults:
            mf.stage_regularize(0, b, mult)
            got.append(mf.stage_get_mvs(0, b).astype(np.int32))
        if [H.sha256_of(v.astype(np.int16)) for v in got] != rec["sweeps"]:
            pytest.fail(sweep_failure(oracle, p1[0], p2[0], g["search"][0], g["block"][0], b, field, mults, got, what))
    mf.close()


@pytest.mark.parametrize("form", list(H.REF_SWEEP_FORMS))
@pytest.mark.parametrize("b", [16, 8, 2])
def test_int16_bound_vectors_against_the_reference(bbme, oracle, b, form):
    """Vectors at int16's bounds: sweeps on level 1 and, at b = 2, the search of level 0 from the coarse grid (copyMVs doubles it)."""
    g = H.INT16_LEVELS
    B0, B1 = g["block"]
    p1, p2, field = H.int16_case(b)
    rec = DIGESTS["sweeps"]["int16_b%d" % b]
    what = "int16 b=%d %s" % (b, form)
    assert H.sha256_of(p1[0], p2[0], p1[1], p2[1], field) == rec["inputs"], INPUT_MISMATCH % what
    with knobs(H.REF_SWEEP_FORMS[form]):
        mf = H.make_mf_from_planes(bbme, p1, p2, g["search"], g["block"])
    mf.stage_set_mvs(1, b, field)
    got = []
    for mult in (1, 2):
        mf.stage_regularize(1, b, mult)
        got.append(mf.stage_get_mvs(1, b).astype(np.int32))
    if [H.sha256_of(v.astype(np.int16)) for v in got] != rec["sweeps"]:
        pytest.fail(sweep_failure(oracle, p1[1], p2[1], g["search"][1], B1, b, field, (1, 2), got, what))
    if b == 2:
        for key, grid in (("int16_from_field", field), ("int16_from_sweeps", got[1].astype(np.int16))):
            mf.stage_set_mvs(1, 2, grid)
            mf.stage_search(0)
            v = mf.stage_get_mvs(0, B0).astype(np.int16)
            if H.sha256_of(v) != DIGESTS["coarse"][key]:
                msg = "%s %s: level 0's search from the coarse grid differs from the reference's record" % (what, key)
                if oracle.have_mf_ref():
                    e = oracle.ref_search_from_coarse(p1, p2, g["search"], g["block"], grid).astype(np.int32)
                    bad = np.argwhere((e != v).any(-1))
                    msg += ": %d blocks, first at %s: mf_ref %s gpu %s" % (len(bad), bad[0], e[tuple(bad[0])], v[tuple(bad[0])])
                pytest.fail(msg)
    mf.close()


def test_motion_compensation_against_the_reference(bbme, oracle):
    """MF.draw_MVimage and compensation_error after an estimate against MF::draw_MVimage (:887-905) of the reference on the
    grid the reference's own schedule left, per level, at 2 x 2, 8 x 8 and the level's own blocks."""
    name = H.REF_MC_CASE
    p1, p2, search, block, raster = H.ref_stage_case(oracle, name)
    assert input_digest(p1, p2, search, block) == DIGESTS["stages"][name]["inputs"], INPUT_MISMATCH % name
    mf = H.make_mf_from_planes(bbme, p1, p2, search, block, raster)
    flow = mf.calcMotionBlockMatching()
    assert H.sha256_of(flow.astype(np.float32)) == DIGESTS["stages"][name]["flow"]
    for lvl in range(len(block)):
        h, w = p1[lvl].shape
        for b in sorted({2, 8, block[lvl]}):
            rec = DIGESTS["mc"]["l%d_b%d" % (lvl, b)]
            frames = [mf.draw_MVimage(lvl, b, fill) for fill in H.REF_MC_FILLS]
            for fill, frame, digest in zip(H.REF_MC_FILLS, frames, rec["frames"]):
                if H.sha256_of(frame) != digest:
                    msg = "level %d block %d fill %d: the frame differs from the reference's draw_MVimage" % (lvl, b, fill)
                    if oracle.have_mf_ref():
                        e = oracle.ref_mc(p2[lvl], b, mf.stage_get_mvs(lvl, 2)[::b // 2, ::b // 2], fill)
                        bad = np.argwhere(e != frame)
                        msg += ": %d pixels (on the kernels' own grid), first at %s" % (len(bad), bad[0] if len(bad) else None)
                    pytest.fail(msg)
            st = mf.compensation_error(lvl, b, window=(0, 0, w, h))
            assert [st["sse"], st["sad"], st["pixels"], st["skipped"]] == rec["stats"], (lvl, b, st)
    mf.close()
