"""Chain contexts (bbme_create_chain: the consecutive pairs of a video over shared frame slots) -- what can be checked without
a GPU: the C-ABI's symbols and argument checks, the segment plan of a video and its frame count, the synthetic video."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

CHAIN_SYMBOLS = ("bbme_create_chain", "bbme_chain_frames", "bbme_set_chain_frames_host", "bbme_set_chain_frames_host_async",
                 "bbme_set_chain_frames_device", "bbme_chain_advance")
MAX_BATCH = 64


def test_chain_symbols_are_exported_declared_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bbme.h")).read(), flags=re.S)
    assert "#define BBME_MAX_BATCH %d" % MAX_BATCH in header
    raw = C.CDLL(_capi.LIB_PATH)
    for name in CHAIN_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in bbme.h"
        assert hasattr(raw, name), name + " is not exported"
        assert name in _capi.SIGNATURES and _capi.SIGNATURES[name][0] is C.c_int, name + " is not bound"
    for name in ("MFChain", "synth_video"):
        assert hasattr(bbme, name) and name in bbme.__all__


def test_chain_calls_refuse_a_null_context(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    n = C.c_int(-7)
    table = (C.c_void_p * 1)(1)
    calls = {"bbme_chain_frames": lambda: lib.bbme_chain_frames(None, C.byref(n)),
             "bbme_set_chain_frames_host": lambda: lib.bbme_set_chain_frames_host(None, 0, 1, table, 64, 1),
             "bbme_set_chain_frames_host_async": lambda: lib.bbme_set_chain_frames_host_async(None, 0, 1, table, 64, 1),
             "bbme_set_chain_frames_device": lambda: lib.bbme_set_chain_frames_device(None, 0, 1, table, 64, 1),
             "bbme_chain_advance": lambda: lib.bbme_chain_advance(None)}
    for name, call in calls.items():
        assert call() == _capi.ERR_INVALID, name
        assert lib.bbme_last_error(), name


def test_create_chain_validates_before_it_looks_for_a_device(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    params = _capi.make_params([30, 30], [16, 16])
    ctx = C.c_void_p()
    for pairs in (0, -1, MAX_BATCH + 1):
        assert lib.bbme_create_chain(C.byref(params), 128, 128, 0, pairs, C.byref(ctx)) == _capi.ERR_INVALID, pairs
        assert not ctx.value and lib.bbme_last_error()
    assert lib.bbme_create_chain(None, 128, 128, 0, 2, C.byref(ctx)) == _capi.ERR_INVALID
    assert lib.bbme_create_chain(C.byref(params), 128, 128, 0, 2, None) == _capi.ERR_INVALID
    bad = _capi.make_params([30, 30], [16, 12])              # not a power of two: refused as bbme_create_batch refuses it
    assert lib.bbme_create_chain(C.byref(bad), 128, 128, 0, 2, C.byref(ctx)) == \
        lib.bbme_create_batch(C.byref(bad), 128, 128, 0, 2, C.byref(ctx)) != _capi.OK
    z = np.zeros((40, 48), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MFChain([z], [30, 30], [16, 16])                # one frame is no pair
    assert e.value.status == _capi.ERR_INVALID
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MFChain([z, z], [30, 30], [16, 16], upsample=2)
    assert e.value.status == _capi.ERR_INVALID


def test_chain_has_no_cpu_fallback_without_device(bbme):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    params = _capi.make_params([30, 30], [16, 16])
    ctx = C.c_void_p()
    for pairs in (1, 2, MAX_BATCH):
        assert lib.bbme_create_chain(C.byref(params), 128, 128, 0, pairs, C.byref(ctx)) == _capi.ERR_HIP
        assert b"no CPU fallback" in lib.bbme_last_error() and not ctx.value
    z = np.zeros((128, 128), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MFChain([z, z, z], [30, 30], [16, 16])
    assert e.value.status == _capi.ERR_HIP and "no CPU fallback" in e.value.message


def test_plan_frame_segments_sets_every_frame_once(bbme):
    from blockbasedmotionestimation_amd.sequence import plan_frame_segments
    for n_pairs in range(1, 41):
        for slots in range(1, 6):
            for batch in range(1, 7):
                what = "n_pairs %d, slots %d, batch %d" % (n_pairs, slots, batch)
                rounds = plan_frame_segments(n_pairs, slots, batch)
                covered = []
                per_slot = {}
                for slot, first, count, carry in rounds:
                    assert 0 <= slot < slots and 1 <= count <= batch, what
                    covered += list(range(first, first + count))
                    per_slot.setdefault(slot, []).append((first, count, carry))
                assert sorted(covered) == list(range(n_pairs)), what          # every pair in exactly one round
                lengths = []
                for slot, rs in per_slot.items():
                    for i, (first, count, carry) in enumerate(rs):
                        assert carry == (i > 0), what                         # false exactly on a slot's first round
                        if i:
                            assert first == rs[i - 1][0] + rs[i - 1][1], what  # contiguous and ascending
                    lengths.append(sum(r[1] for r in rs))
                assert len(per_slot) == min(slots, n_pairs) and max(lengths) - min(lengths) <= 1, what
                # segments lie in the video's order, slot after slot
                starts = [per_slot[s][0][0] for s in sorted(per_slot)]
                assert starts == sorted(starts) and sorted(per_slot) == list(range(len(per_slot))), what
                # the halving: a round sets `count` frames, one more when nothing is carried -- against two per pair
                frames_set = sum(count + (0 if carry else 1) for _, _, count, carry in rounds)
                assert frames_set == n_pairs + len(per_slot), what
                assert frames_set <= 2 * n_pairs, what
                # issue order: round-robin over the slots that still have pairs
                seen = {}
                for k, (slot, _, _, _) in enumerate(rounds):
                    seen.setdefault(slot, []).append(k)
                first_round = [seen[s][0] for s in sorted(seen)]
                assert first_round == list(range(len(seen))), what
    assert plan_frame_segments(0, 3, 2) == []
    with pytest.raises(ValueError):
        plan_frame_segments(4, 0, 2)
    with pytest.raises(ValueError):
        plan_frame_segments(4, 2, 0)


def test_shard_frames_covers_every_pair_once_contiguously(bbme):
    from blockbasedmotionestimation_amd.sequence import plan_frame_segments, shard_frames
    for world in range(1, 9):
        for n_frames in range(0, 30):
            n_pairs = max(n_frames - 1, 0)
            shards = [shard_frames(n_frames, r, world) for r in range(world)]
            pairs, nxt = [], 0
            for s in shards:
                if s is None:
                    continue
                first, last = s
                assert first == nxt and last > first                           # contiguous over the ranks, never empty
                pairs += list(range(first, last))
                nxt = last
            assert pairs == list(range(n_pairs)), (world, n_frames)
            sizes = [0 if s is None else s[1] - s[0] for s in shards]
            assert max(sizes) - min(sizes) <= 1
            # one round per rank of plan_frame_segments
            if n_pairs:
                plan = plan_frame_segments(n_pairs, world, n_pairs)
                assert [(f, f + c) for _, f, c, _ in plan] == [s for s in shards if s is not None]


def test_synth_video_is_seeded_and_moves(bbme):
    a = bbme.synth_video(96, 64, 5, 11, max_motion=4)
    b = bbme.synth_video(96, 64, 5, 11, max_motion=4)
    c = bbme.synth_video(96, 64, 5, 12, max_motion=4)
    assert len(a) == 5
    for f in a:
        assert f.dtype == np.uint8 and f.shape == (64, 96)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not any(np.array_equal(x, y) for x, y in zip(a, c))
    for k in range(4):
        assert not np.array_equal(a[k], a[k + 1])
    # without motion and noise nothing changes from frame to frame; with motion only, tiles are shifted copies
    still = bbme.synth_video(96, 64, 3, 5, max_motion=0, noise=0)
    assert np.array_equal(still[0], still[1]) and np.array_equal(still[1], still[2])
    one = bbme.synth_video(64, 64, 2, 9, max_motion=3, tiles=1, noise=0)
    hits = [(dx, dy) for dx in range(-3, 4) for dy in range(-3, 4)
            if np.array_equal(one[1][8 + dy:56 + dy, 8 + dx:56 + dx], one[0][8:56, 8:56])]
    assert len(hits) >= 1
    assert len(bbme.synth_video(32, 32, 1, 3)) == 1
    with pytest.raises(ValueError):
        bbme.synth_video(32, 32, 0, 3)
