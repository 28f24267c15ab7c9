"""Chain contexts on the GPU (bbme_create_chain, MFChain): P consecutive pairs of a video over P + 1 frame slots, every frame
set once.  The feature moves bytes and pointers and computes nothing new, so every comparison here is bit for bit: a chain's
planes, cells, fields, compensated frames and statistics against an MF of its own on (f_p, f_p+1), and once against the CPU
oracle so that the check is not only the library against itself."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# parameter sets of tests/test_gpu_parity.py::CASES
MIXED = (320, 256, [24, 40, 30], [8, 16, 8])          # another block / search size per level
STRIP = (512, 384, [80, 80, 80], [16, 16, 16])        # +-32 at 16 x 16: the strip search kernel, windows leave the image
B8 = (256, 256, [72, 72], [8, 8])                     # 8 x 8 blocks, +-32
PADDED = (200, 120, [30, 30], [16, 16])               # padded in both dimensions (224 x 128)
SETS = {"mixed": MIXED, "strip_r32": STRIP, "b8": B8}

ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -7, -8


def _video(bbme, w, h, n, seed, mm=6):
    return bbme.synth_video(w, h, n, seed, max_motion=mm)


def _own(bbme, f1, f2, search, block, upsample=1, what="cells"):
    """What an MF of its own makes of one pair."""
    mf = bbme.MF(f1, f2, search, block, upsample=upsample)
    mf.estimate_async()
    out = dict(cells=mf.get_cells(), flow=mf.get_flow())
    if what == "all":
        out["sub"] = mf.get_subsampled_flow()
        out["mc"] = mf.draw_MVimage()
        out["mc_coarse"] = mf.draw_MVimage(level=mf.num_levels - 1, block=4, fill=9)
        out["err"] = mf.compensation_error()
        out["err_coarse"] = mf.compensation_error(level=mf.num_levels - 1, block=4)
    mf.close()
    return out


def _assert_pairs(bbme, chain, frames, search, block, what, upsample=1, expect=None):
    for p in range(len(frames) - 1):
        exp = expect[p] if expect is not None else _own(bbme, frames[p], frames[p + 1], search, block, upsample)["cells"]
        assert np.array_equal(chain.get_pair_cells(p), exp), "%s: cells of pair %d" % (what, p)


def _status(lib, call):
    """(status, message) of a C-ABI call."""
    rc = call()
    return rc, lib.bbme_last_error()


# ---- planes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,search,block,upsample", [
    PADDED + (1,),                                      # zero border in both dimensions
    (100, 60, [12, 12], [4, 4], 1),                     # level widths 104 / 52: a level width that is not a multiple of 8 (see below)
    (100, 60, [12, 12, 12], [4, 4, 4], 1),              # 112 / 56 / 28
    (50, 30, [30, 30], [16, 16], 4),                    # original frames, up-sampled x4 on the GPU
    (37, 29, [30, 30], [16, 16], 4),                    # odd source size: pad_x % 4 = 2
], ids=["padded", "w104_52", "w112_56_28", "x4", "x4_odd"])
def test_chain_of_one_pair_has_the_planes_of_an_mf(bbme, w, h, search, block, upsample):
    """bbme_get_level_planes_host of a chain of one pair (slot 0, slot 1) on every level against an MF on the same two frames.
    A context only accepts geometries whose every level width is a multiple of 4, so a level that is pyrDown's SOURCE is always
    a multiple of 8 wide (what k_pyr_down4_run needs) and only the coarsest level can be anything else (52 and 28 here)."""
    widths = [bbme.plan_padding(w * upsample, h * upsample, search, block)[0] >> l for l in range(len(block))]
    assert all(x % 8 == 0 for x in widths[:-1]) and widths[-1] % 4 == 0
    if (w, upsample) == (100, 1):
        assert widths == ([104, 52] if len(block) == 2 else [112, 56, 28])
    rng = np.random.default_rng(w * 31 + h)
    f = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2)]
    mf = bbme.MF(f[0], f[1], search, block, upsample=upsample)
    chain = bbme.MFChain(f, search, block, upsample=upsample)
    assert chain.batch == 1 and chain.slots == 2
    assert (chain.padded_width, chain.padded_height, chain.padding_x, chain.padding_y) == \
           (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y)
    for l in range(len(block)):
        (a, b), (ea, eb) = chain.get_level_planes(l), mf.get_level_planes(l)
        assert np.array_equal(a, ea) and np.array_equal(b, eb), "level %d" % l
        # the getter by slot (the only one a chain of more than one pair has) reads the same bytes
        assert np.array_equal(chain.get_slot_plane(l, 0), ea) and np.array_equal(chain.get_slot_plane(l, 1), eb), "level %d" % l
    plane = np.zeros((mf.padded_height, mf.padded_width), np.uint8)
    for ctx, level, slot, status in ((chain._ctx, 0, 2, ERR_INVALID), (chain._ctx, 0, -1, ERR_INVALID), (chain._ctx, len(block), 0, ERR_INVALID),
                                     (mf._ctx, 0, 0, ERR_UNSUPPORTED)):
        assert chain._lib.bbme_get_chain_plane_host(ctx, level, slot, plane.ctypes.data) == status, (level, slot)
    assert chain._lib.bbme_get_chain_plane_host(chain._ctx, 0, 0, None) == ERR_INVALID
    # a run of one frame into either slot
    g = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2)]
    mf.set_frames(g[0], f[1])
    chain.set_frame_run(0, [g[0]])
    for l in range(len(block)):
        (a, b), (ea, eb) = chain.get_level_planes(l), mf.get_level_planes(l)
        assert np.array_equal(a, ea) and np.array_equal(b, eb), "slot 0 again, level %d" % l
    mf.set_frames(g[0], g[1])
    chain.set_frame_run(1, [g[1]], wait=False)
    for l in range(len(block)):
        (a, b), (ea, eb) = chain.get_level_planes(l), mf.get_level_planes(l)
        assert np.array_equal(a, ea) and np.array_equal(b, eb), "slot 1 again (async), level %d" % l
    chain.close()
    mf.close()


# ---- fields -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
@pytest.mark.parametrize("pairs", [1, 2, 5])
@pytest.mark.parametrize("name", sorted(SETS))
def test_every_pair_of_a_chain_equals_its_own_mf(bbme, monkeypatch, name, pairs, no_graph):
    w, h, search, block = SETS[name]
    if no_graph:
        monkeypatch.setenv("BBME_NO_GRAPH", "1")
    frames = _video(bbme, w, h, pairs + 1, 7000 + 10 * pairs + len(name))
    chain = bbme.MFChain(frames, search, block)
    assert chain.batch == pairs and chain.slots == pairs + 1
    exp = [_own(bbme, frames[p], frames[p + 1], search, block) for p in range(pairs)]
    for run in ("first", "again"):                       # the second estimate replays the captured graph
        chain.estimate_async()
        for p in range(pairs):
            assert np.array_equal(chain.get_pair_cells(p), exp[p]["cells"]), "%s: cells of pair %d" % (run, p)
    for p in range(pairs):
        assert np.array_equal(chain.get_pair_flow(p), exp[p]["flow"]), "flow of pair %d" % p
    chain.close()


def test_chain_against_the_cpu_oracle(bbme, oracle):
    w, h, search, block = MIXED
    frames = _video(bbme, w, h, 4, 7100)
    chain = bbme.MFChain(frames, search, block)
    got = chain.calcMotionBlockMatching()
    chain.close()
    for p in range(3):
        omf = oracle.OracleMF(frames[p], frames[p + 1], search, block)
        assert np.array_equal(got[p], omf.calc_motion_block_matching()), "pair %d" % p
        omf.close()


@pytest.mark.parametrize("name", ["strip_r32", "b8"])
def test_chain_of_one_pair_with_every_level_speculated(bbme, monkeypatch, name):
    w, h, search, block = SETS[name]
    monkeypatch.setenv("BBME_SPEC_MIN_GABS", "0")
    monkeypatch.setenv("BBME_SPECULATE", "1")
    frames = _video(bbme, w, h, 2, 7200, mm=12)
    chain = bbme.MFChain(frames, search, block)
    chain.set_speculation(True)
    monkeypatch.delenv("BBME_SPEC_MIN_GABS")
    monkeypatch.setenv("BBME_SPECULATE", "0")
    exp = _own(bbme, frames[0], frames[1], search, block)["cells"]
    for run in range(2):
        chain.estimate_async()
        assert np.array_equal(chain.get_pair_cells(0), exp), "run %d" % run
    chain.close()


# ---- rolling ----------------------------------------------------------------------------------------------------------

def test_rolling_through_a_video(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    w, h, search, block = MIXED
    P = 2
    frames = _video(bbme, w, h, 1 + 3 * P, 7300)
    exp = [_own(bbme, frames[p], frames[p + 1], search, block)["cells"] for p in range(3 * P)]
    chain = bbme.MFChain(frames[:P + 1], search, block)
    stats = (C.c_ulonglong * (4 * P))()
    for rnd in range(3):
        if rnd:
            prev = [chain.get_pair_cells(p) for p in range(P)]
            _capi.check(lib.bbme_chain_advance(chain._ctx))
            # slots 1 .. P are unset: nothing that reads planes may run; what the last estimate left stays readable
            for what, call in (("estimate", lambda: lib.bbme_estimate(chain._ctx)),
                               ("compensation_error", lambda: lib.bbme_compensation_error(chain._ctx, 0, 2, None, stats))):
                rc, msg = _status(lib, call)
                assert rc == ERR_STATE and msg, "%s after advance" % what
            for p in range(P):
                assert np.array_equal(chain.get_pair_cells(p), prev[p]), "cells of the previous round, pair %d" % p
            chain.set_frame_run(1, frames[rnd * P + 1:rnd * P + 2])          # all but the last slot
            for what, call in (("estimate", lambda: lib.bbme_estimate(chain._ctx)),
                               ("compensation_error", lambda: lib.bbme_compensation_error(chain._ctx, 0, 2, None, stats))):
                rc, msg = _status(lib, call)
                assert rc == ERR_STATE and msg, "%s before the last slot is set" % what
            chain.set_frame_run(2, frames[rnd * P + 2:rnd * P + 3])
        chain.estimate_async()
        for p in range(P):
            assert np.array_equal(chain.get_pair_cells(p), exp[rnd * P + p]), "round %d, pair %d" % (rnd, p)
    chain.close()


@pytest.mark.parametrize("name,pairs", [("strip_r32", 2), ("mixed", 3)])
def test_six_rounds_on_one_context_with_a_live_sad_memo(bbme, name, pairs):
    """Levels of 16 x 16 blocks: their sweeps run with the SAD memo, which every frame setter and the roll must reset."""
    w, h, search, block = SETS[name]
    assert max(block) >= 16
    frames = _video(bbme, w, h, 1 + 6 * pairs, 7400 + pairs)
    chain = bbme.MFChain(frames[:pairs + 1], search, block)
    for rnd in range(6):
        if rnd:
            chain.advance(frames[rnd * pairs + 1:(rnd + 1) * pairs + 1], wait=bool(rnd & 1))
        chain.estimate_async()
        _assert_pairs(bbme, chain, frames[rnd * pairs:(rnd + 1) * pairs + 1], search, block, "round %d" % rnd)
    chain.close()


def test_resetting_one_slot_changes_its_two_pairs_only(bbme):
    w, h, search, block = MIXED
    P = 4
    frames = _video(bbme, w, h, P + 1, 7500)
    other = _video(bbme, w, h, P + 1, 7501)
    chain = bbme.MFChain(frames, search, block)
    chain.estimate_async()
    before = [chain.get_pair_cells(p) for p in range(P)]
    for k in (2, 0, P):
        cur = list(frames)
        cur[k] = other[k]
        chain.set_frame_run(0, frames)
        chain.set_frame_run(k, [other[k]])
        chain.estimate_async()
        for p in range(P):
            got = chain.get_pair_cells(p)
            if p in (k - 1, k):
                exp = _own(bbme, cur[p], cur[p + 1], search, block)["cells"]
                assert np.array_equal(got, exp), "slot %d: pair %d" % (k, p)
                assert not np.array_equal(got, before[p]), "slot %d: pair %d did not change" % (k, p)
            else:
                assert np.array_equal(got, before[p]), "slot %d: pair %d changed" % (k, p)
    chain.close()


# ---- device frames ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("upsample", [1, 4])
def test_device_frames_with_a_row_pitch(bbme, upsample):
    import torch
    w, h, search, block = (80, 64, [30, 30], [16, 16]) if upsample == 4 else MIXED
    P = 3
    frames = _video(bbme, w, h, 2 * P + 1, 7600 + upsample, mm=3 if upsample == 4 else 6)
    staged = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()

    def produce(idx):
        """Strided tensors written on torch's current stream just before they are handed over."""
        out = []
        for i in idx:
            big = torch.empty((h, w + 13), dtype=torch.uint8, device="cuda")
            big.fill_(0xEE)
            big[:, :w].copy_(staged[i], non_blocking=True)
            out.append(big[:, :w])
        assert out[0].stride(0) == w + 13
        return out
    with torch.cuda.stream(torch.cuda.Stream()):
        chain = bbme.MFChain(produce(range(P + 1)), search, block, frames_on_device=True, upsample=upsample)
        chain.estimate_async()
        for rnd in range(2):
            if rnd:
                chain.advance(produce(range(P + 1, 2 * P + 1)))
                chain.estimate_async()
            for p in range(P):
                q = rnd * P + p
                mf = bbme.MF(frames[q], frames[q + 1], search, block, upsample=upsample)
                mf.estimate_async()
                assert np.array_equal(chain.get_pair_cells(p), mf.get_cells()), "round %d, pair %d" % (rnd, p)
                assert np.array_equal(chain.get_pair_subsampled_flow(p), mf.get_subsampled_flow()), "round %d, pair %d" % (rnd, p)
                mf.close()
    with pytest.raises(bbme.BbmeError) as e:                # a host array on a device-frame context, a tensor of another size
        chain.set_frame_run(0, [frames[0]])
    assert e.value.status == ERR_INVALID
    with pytest.raises(bbme.BbmeError) as e:
        chain.set_frame_run(0, [staged[0][:h - 1]])
    assert e.value.status == ERR_INVALID
    chain.close()


# ---- motion compensation ---------------------------------------------------------------------------------------------

def test_motion_compensation_of_a_chain(bbme):
    w, h, search, block = PADDED
    P = 3
    frames = _video(bbme, w, h, P + 1, 7700)
    chain = bbme.MFChain(frames, search, block)
    chain.estimate_async()
    errs = chain.compensation_errors()
    errs_coarse = chain.compensation_errors(level=chain.num_levels - 1, block=4)
    assert len(errs) == P
    for p in range(P):
        exp = _own(bbme, frames[p], frames[p + 1], search, block, what="all")
        assert np.array_equal(chain.get_pair_motion_compensated(p), exp["mc"]), "pair %d" % p
        assert np.array_equal(chain.get_pair_motion_compensated(p, level=chain.num_levels - 1, block=4, fill=9), exp["mc_coarse"])
        assert errs[p] == exp["err"] and errs_coarse[p] == exp["err_coarse"], "pair %d" % p
        assert errs[p]["pixels"] > 0
    chain.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_refusals(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    w, h, search, block = PADDED
    frames = _video(bbme, w, h, 4, 7800)
    f = [np.ascontiguousarray(x) for x in frames]
    ptr = [x.ctypes.data for x in f]
    dev = [torch.from_numpy(x).cuda() for x in f]
    dptr = [t.data_ptr() for t in dev]
    torch.cuda.synchronize()

    def table(*ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def expect(rc_expected, what, call):
        rc, msg = _status(lib, call)
        assert rc == rc_expected and msg, "%s: status %d, message %r" % (what, rc, msg)

    params = _capi.make_params(search, block)
    ctx = C.c_void_p()
    _capi.check(lib.bbme_create_chain(C.byref(params), w, h, 0, 3, C.byref(ctx)))
    n = C.c_int()
    _capi.check(lib.bbme_batch_size(ctx, C.byref(n)))
    assert n.value == 3
    _capi.check(lib.bbme_chain_frames(ctx, C.byref(n)))
    assert n.value == 4
    expect(ERR_INVALID, "chain_frames, null output", lambda: lib.bbme_chain_frames(ctx, None))
    stats = (C.c_ulonglong * 12)()
    plane = np.zeros((512, 512), np.uint8)
    # nothing set yet
    expect(ERR_STATE, "estimate before frames", lambda: lib.bbme_estimate(ctx))
    # the pair setters
    for name in ("bbme_set_frames_host_pair", "bbme_set_frames_host_async", "bbme_set_frames_device_pair", "bbme_set_frames_host_x4",
                 "bbme_set_frames_host_x4_async", "bbme_set_frames_device_x4"):
        src = dptr if "device" in name else ptr
        expect(ERR_UNSUPPORTED, name, lambda: getattr(lib, name)(ctx, 0, src[0], src[1], w))
    expect(ERR_UNSUPPORTED, "bbme_set_frames_host", lambda: lib.bbme_set_frames_host(ctx, ptr[0], ptr[1], w))
    expect(ERR_UNSUPPORTED, "bbme_set_frames_device", lambda: lib.bbme_set_frames_device(ctx, dptr[0], dptr[1], w))
    # bad runs
    for name in ("bbme_set_chain_frames_host", "bbme_set_chain_frames_host_async", "bbme_set_chain_frames_device"):
        fn = getattr(lib, name)
        src = dptr if "device" in name else ptr
        expect(ERR_INVALID, name + ": first < 0", lambda: fn(ctx, -1, 1, table(src[0]), w, 1))
        expect(ERR_INVALID, name + ": first past the slots", lambda: fn(ctx, 4, 1, table(src[0]), w, 1))
        expect(ERR_INVALID, name + ": count 0", lambda: fn(ctx, 0, 0, table(src[0]), w, 1))
        expect(ERR_INVALID, name + ": run past the slots", lambda: fn(ctx, 2, 3, table(*src[:3]), w, 1))
        expect(ERR_INVALID, name + ": null table", lambda: fn(ctx, 0, 1, None, w, 1))
        expect(ERR_INVALID, name + ": null entry", lambda: fn(ctx, 0, 2, table(src[0], None), w, 1))
        expect(ERR_INVALID, name + ": pitch", lambda: fn(ctx, 0, 1, table(src[0]), w - 1, 1))
        expect(ERR_INVALID, name + ": pitch of a x4 run", lambda: fn(ctx, 0, 1, table(src[0]), w // 4 - 1, 4))
        for scale in (0, 2, 3, 8):
            expect(ERR_INVALID, name + ": scale %d" % scale, lambda: fn(ctx, 0, 1, table(src[0]), w, scale))
    # three of four slots
    _capi.check(lib.bbme_set_chain_frames_host(ctx, 0, 3, table(*ptr[:3]), w, 1))
    expect(ERR_STATE, "estimate with a slot unset", lambda: lib.bbme_estimate(ctx))
    _capi.check(lib.bbme_set_chain_frames_device(ctx, 3, 1, table(dptr[3]), w, 1))
    _capi.check(lib.bbme_estimate(ctx))
    _capi.check(lib.bbme_synchronize(ctx))
    _capi.check(lib.bbme_compensation_error(ctx, 0, 2, None, stats))
    # single-pair calls on a chain of three pairs, as on a batch
    expect(ERR_UNSUPPORTED, "stage_search", lambda: lib.bbme_stage_search(ctx, 0))
    expect(ERR_UNSUPPORTED, "level planes", lambda: lib.bbme_get_level_planes_host(ctx, 0, plane.ctypes.data, plane.ctypes.data))
    # after the roll
    _capi.check(lib.bbme_chain_advance(ctx))
    expect(ERR_STATE, "estimate after advance", lambda: lib.bbme_estimate(ctx))
    expect(ERR_STATE, "compensation_error after advance", lambda: lib.bbme_compensation_error(ctx, 0, 2, None, stats))
    expect(ERR_STATE, "get_motion_compensated after advance",
           lambda: lib.bbme_get_motion_compensated_host(ctx, 0, 0, 2, 0, plane.ctypes.data))
    out = torch.empty((512, 512), dtype=torch.uint8, device="cuda")
    expect(ERR_STATE, "motion_compensate_device after advance",
           lambda: lib.bbme_motion_compensate_device(ctx, 0, 0, 2, 0, C.c_void_p(out.data_ptr()), 512, None))
    expect(ERR_INVALID, "compensation_error, bad level", lambda: lib.bbme_compensation_error(ctx, 9, 2, None, stats))
    _capi.check(lib.bbme_destroy(ctx))

    # a chain of one pair: the stage calls refuse while a slot is unset
    _capi.check(lib.bbme_create_chain(C.byref(params), w, h, 0, 1, C.byref(ctx)))
    _capi.check(lib.bbme_set_chain_frames_host(ctx, 0, 1, table(ptr[0]), w, 1))
    expect(ERR_STATE, "stage_search with slot 1 unset", lambda: lib.bbme_stage_search(ctx, 1))
    expect(ERR_STATE, "stage_regularize with slot 1 unset", lambda: lib.bbme_stage_regularize(ctx, 1, 16, 1))
    _capi.check(lib.bbme_set_chain_frames_host(ctx, 1, 1, table(ptr[1]), w, 1))
    _capi.check(lib.bbme_stage_search(ctx, 1))
    _capi.check(lib.bbme_chain_advance(ctx))
    expect(ERR_STATE, "stage_search after advance", lambda: lib.bbme_stage_search(ctx, 1))
    _capi.check(lib.bbme_destroy(ctx))

    # x4 runs need a context whose size is a multiple of 4
    _capi.check(lib.bbme_create_chain(C.byref(params), 202, 120, 0, 1, C.byref(ctx)))
    expect(ERR_INVALID, "x4 run on a 202-wide context", lambda: lib.bbme_set_chain_frames_host(ctx, 0, 1, table(ptr[0]), 202, 4))
    _capi.check(lib.bbme_destroy(ctx))

    # the chain calls on contexts that are no chain
    for pairs in (1, 2):
        _capi.check(lib.bbme_create_batch(C.byref(params), w, h, 0, pairs, C.byref(ctx)))
        _capi.check(lib.bbme_chain_frames(ctx, C.byref(n)))
        assert n.value == 0
        expect(ERR_UNSUPPORTED, "advance", lambda: lib.bbme_chain_advance(ctx))
        expect(ERR_UNSUPPORTED, "chain host", lambda: lib.bbme_set_chain_frames_host(ctx, 0, 1, table(ptr[0]), w, 1))
        expect(ERR_UNSUPPORTED, "chain host async", lambda: lib.bbme_set_chain_frames_host_async(ctx, 0, 1, table(ptr[0]), w, 1))
        expect(ERR_UNSUPPORTED, "chain device", lambda: lib.bbme_set_chain_frames_device(ctx, 0, 1, table(dptr[0]), w, 1))
        _capi.check(lib.bbme_destroy(ctx))

    # the Python layer
    chain = bbme.MFChain(frames[:3], search, block)
    for call in (lambda: chain.set_pair(0, frames[0], frames[1]), lambda: chain.set_frames(frames[0], frames[1]),
                 lambda: chain.set_pair_device(0, dev[0], dev[1])):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == ERR_UNSUPPORTED and e.value.message
    for call in (lambda: chain.set_frame_run(2, frames[:2]), lambda: chain.set_frame_run(-1, frames[:1]),
                 lambda: chain.set_frame_run(0, []), lambda: chain.set_frame_run(0, [frames[0][:-1]])):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == ERR_INVALID
    chain.close()


def test_a_chain_of_64_pairs_has_65_slots(bbme):
    """64 pairs are 65 frame slots: one more than a 64-bit word of flags would hold."""
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    search, block = [30, 30], [16, 16]
    frames = _video(bbme, 96, 64, 65, 7900, mm=3)
    chain = bbme.MFChain(frames[:64] + [frames[63]], search, block)      # 65 slots, the last one to be replaced
    assert chain.batch == 64 and chain.slots == 65
    chain.set_frame_run(64, [frames[64]])
    chain.estimate_async()
    for p in (0, 31, 62, 63):
        assert np.array_equal(chain.get_pair_cells(p), _own(bbme, frames[p], frames[p + 1], search, block)["cells"]), "pair %d" % p
    _capi.check(lib.bbme_chain_advance(chain._ctx))
    assert lib.bbme_estimate(chain._ctx) == ERR_STATE
    chain.set_frame_run(1, frames[:63])
    assert lib.bbme_estimate(chain._ctx) == ERR_STATE                     # slot 64 alone is unset
    chain.set_frame_run(64, [frames[0]])
    chain.estimate_async()
    assert np.array_equal(chain.get_pair_cells(0), _own(bbme, frames[64], frames[0], search, block)["cells"])
    assert np.array_equal(chain.get_pair_cells(63), _own(bbme, frames[62], frames[0], search, block)["cells"])
    chain.close()


# ---- the pipeline -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames", [1, 2, 7, 11])
def test_frames_pipeline_equals_the_pair_pipeline(bbme, n_frames):
    from blockbasedmotionestimation_amd.sequence import estimate_frames_pipelined, estimate_pairs_pipelined
    w, h, search, block = 328, 200, [40, 40, 40], [8, 8, 8]
    frames = _video(bbme, w, h, n_frames, 8000 + n_frames)
    for k, per in ((1, 1), (4, 2), (6, 3)):
        exp = estimate_pairs_pipelined(list(zip(frames, frames[1:])), search, block, in_flight=k, batch=per)
        got = estimate_frames_pipelined(frames, search, block, in_flight=k, batch=per)
        assert len(got) == len(exp) == n_frames - 1
        for p, (g, e) in enumerate(zip(got, exp)):
            assert g.shape == (h, w, 2) and g.dtype == np.float32 and np.array_equal(g, e), "pair %d (%d, %d)" % (p, k, per)
    assert estimate_frames_pipelined([], search, block) == []


def test_frames_pipeline_with_upsampling(bbme):
    from blockbasedmotionestimation_amd.sequence import estimate_frames_pipelined, estimate_pairs_pipelined
    w, h, search, block = 82, 50, [30, 30], [16, 16]
    frames = _video(bbme, w, h, 6, 8100, mm=2)
    big = [bbme.resize_x4(f) for f in frames]
    exp = estimate_pairs_pipelined(list(zip(big, big[1:])), search, block, in_flight=4, batch=2)
    got = estimate_frames_pipelined(frames, search, block, in_flight=4, batch=2, upsample=4)
    assert len(got) == 5
    for p, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == (4 * h, 4 * w, 2) and np.array_equal(g, e), "pair %d" % p
