"""Chain contexts (bbme_create_chain: the consecutive pairs of a video over shared frame slots) -- what can be checked without
a GPU: the C-ABI's symbols and argument checks, the segment plan of a video and its frame count, the synthetic video, and the
walk of the video drivers over their chain contexts (collect before advance, padding, speculation, close) on a recording fake."""
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


# ---- the video drivers' walk over chain contexts, through the public drivers on a recording fake of MFChain ----------------
WALK_H, WALK_W = 8, 12
WALK_GRID = [(n, i, b) for n in range(2, 14) for i in (1, 2, 4, 6) for b in (1, 2, 3)]


class _FakeChain:
    """Stands in for MFChain: keeps the numbers of the frames it holds (frame i of the video is filled with i), answers every
    read of pair p with an array that encodes the numbers in slots p and p + 1 at the moment of the call, and logs every call.
    fail_round = r: a read of the r-th round issued (counted over all chains) raises."""
    log, fail_round, rounds_issued = None, 0, 0

    def __init__(self, frames, search_size, block_size, num_levels=None, device=0, frames_on_device=False, upsample=1):
        cls = type(self)
        self.id = sum(1 for e in cls.log if e[0] == "new")
        self.held = [int(f.flat[0]) for f in frames]
        self.round = 0
        self.orig_height, self.orig_width, self.padding_y, self.padding_x = WALK_H, WALK_W, 0, 0
        cls.log.append(("new", self.id, tuple(self.held), upsample))

    def _note(self, name, *args):
        type(self).log.append((name, self.id) + args)

    def _pair(self, name, p, *args):
        if self.round == type(self).fail_round:
            self._note("raise", name, p)
            raise RuntimeError("read of round %d" % self.round)
        a, b = self.held[p], self.held[p + 1]
        self._note(name, p, a, b, *args)
        return a, b

    def set_speculation(self, enabled):
        self._note("set_speculation", bool(enabled))

    def advance(self, new_frames, wait=True):
        new = [int(f.flat[0]) for f in new_frames]
        assert len(new) == len(self.held) - 1
        self.held = [self.held[-1]] + new
        self.round = 0
        self._note("advance", tuple(new))

    def _estimate(self, name):
        type(self).rounds_issued += 1
        self.round = type(self).rounds_issued
        self._note(name)

    def estimate_async(self):
        self._estimate("estimate_async")

    def estimate_bidirectional_async(self):
        self._estimate("estimate_bidirectional_async")

    def close(self):
        self._note("close")

    def default_cell_window(self):
        return 0, 0, WALK_W // 2, WALK_H // 2

    def _coded(self, a, b, shape, dtype):
        out = np.empty(shape, dtype)
        out[..., 0], out[..., 1:] = a, b
        return out

    def get_pair_flow(self, p, out=None):
        return self._coded(*self._pair("get_pair_flow", p), (WALK_H, WALK_W, 2), np.float32)

    def get_pair_subpel_cells(self, p, which="forward", out=None):
        return self._coded(*self._pair("get_pair_subpel_cells", p), (WALK_H // 2, WALK_W // 2, 2), np.int16)

    def get_pair_backward_cells(self, p, out=None):
        return self._coded(*self._pair("get_pair_backward_cells", p), (WALK_H // 2, WALK_W // 2, 2), np.int16)

    def consistency(self, which="forward", tol=1, pair=0, out=None):      # column 0: the first frame, the others: the second
        return self._coded(*self._pair("consistency", pair, which, tol), (WALK_H // 2, WALK_W // 2), np.uint8)

    def interpolate_run(self, den, pair=0):
        a, b = self._pair("interpolate_run", pair, den)
        return [self._coded(a, b, (WALK_H, WALK_W), np.uint8) for _ in range(den - 1)]

    def interpolate_run_bgr(self, factor, pair=0):
        a, b = self._pair("interpolate_run_bgr", pair, factor)
        return [self._coded(a, b, (WALK_H, WALK_W, 3), np.uint8) for _ in range(factor - 1)]

    def flow_ranges_all(self, which="forward", scale=None):
        if self.round == type(self).fail_round:
            self._note("raise", "flow_ranges_all", -1)
            raise RuntimeError("read of round %d" % self.round)
        self._note("flow_ranges_all", which, scale, tuple(self.held))
        return np.array([[self.held[p], self.held[p + 1], 0, 0, 0] for p in range(len(self.held) - 1)], np.float32)

    def get_pair_flow_color(self, p, scale=None, maxmotion=-1.0, which="forward", out=None):
        return self._coded(*self._pair("get_pair_flow_color", p, scale, maxmotion), (WALK_H, WALK_W, 3), np.uint8)


def _walk_video(n_frames, colour=False):
    shape = (WALK_H, WALK_W, 3) if colour else (WALK_H, WALK_W)
    return [np.full(shape, i, np.uint8) for i in range(n_frames)]


def _walk_drivers():
    """name -> (run(sequence module, n_frames, in_flight, batch), decode(result) -> [(a, b)] per pair, bidirectional)."""
    kw = dict(search_size=[30, 30], block_size=[16, 16], device=0)

    def flows(res):
        return [(int(f[0, 0, 0]), int(f[0, 0, 1])) for f in res]

    def both(res):
        out = []
        for fwd, bwd, m_f, m_b in res:
            codes = {(int(x[0, 0, 0]), int(x[0, 0, 1])) for x in (fwd, bwd)} | {(int(m[0, 0]), int(m[0, 1])) for m in (m_f, m_b)}
            assert len(codes) == 1
            out.append(codes.pop())
        return out

    def between(factor, decode):
        def dec(res):
            assert len(res) % factor == 1
            out = []
            for p in range(len(res) // factor):
                assert int(res[p * factor].flat[0]) == p                     # the original frames, in place
                codes = {decode(f) for f in res[p * factor + 1:(p + 1) * factor]}
                assert len(codes) == 1
                out.append(codes.pop())
            assert int(res[-1].flat[0]) == len(res) // factor
            return out
        return dec

    def coloured(res):
        images, ranges = res
        assert [(int(r[0]), int(r[1])) for r in ranges] == [(int(i[0, 0, 0]), int(i[0, 0, 1])) for i in images]
        return [(int(i[0, 0, 0]), int(i[0, 0, 1])) for i in images]

    return {
        "pipelined": (lambda s, n, i, b: s.estimate_frames_pipelined(_walk_video(n), in_flight=i, batch=b, **kw), flows, False),
        "subpel": (lambda s, n, i, b: s.estimate_frames_pipelined(_walk_video(n), in_flight=i, batch=b, subpel=True, **kw),
                   flows, False),
        "bidirectional": (lambda s, n, i, b: s.estimate_frames_bidirectional(_walk_video(n), in_flight=i, batch=b, **kw), both, True),
        "interpolate": (lambda s, n, i, b: s.interpolate_frames(_walk_video(n), factor=3, in_flight=i, batch=b, **kw),
                        between(3, lambda f: (int(f[0, 0]), int(f[0, 1]))), True),
        "interpolate_bgr": (lambda s, n, i, b: s.interpolate_frames(_walk_video(n, True), factor=2, in_flight=i, batch=b, **kw),
                            between(2, lambda f: (int(f[0, 0, 0]), int(f[0, 0, 1]))), True),
        "colorize": (lambda s, n, i, b: s.colorize_frames(_walk_video(n), in_flight=i, batch=b, **kw), coloured, False),
    }


def _walk(monkeypatch, driver, n_frames, in_flight, batch, fail_round=0):
    """One driver on the fake: (result or the exception a failing read raised, the fake's log)."""
    import blockbasedmotionestimation_amd.motion_framework as motion_framework
    import blockbasedmotionestimation_amd.sequence as sequence
    fake = type("FakeChain", (_FakeChain,), dict(log=[], fail_round=fail_round, rounds_issued=0))
    monkeypatch.setattr(motion_framework, "MFChain", fake)
    try:
        res = _walk_drivers()[driver][0](sequence, n_frames, in_flight, batch)
    except RuntimeError as e:
        res = e
    return res, fake.log


def walk_grid_log(monkeypatch):
    """The fake's full log of every driver over the grid, as text: the sequence of calls made on every chain."""
    lines = []
    for driver in _walk_drivers():
        for n_frames, in_flight, batch in WALK_GRID:
            lines.append("%s n_frames %d in_flight %d batch %d" % (driver, n_frames, in_flight, batch))
            lines += ["  " + repr(e) for e in _walk(monkeypatch, driver, n_frames, in_flight, batch)[1]]
    return "\n".join(lines) + "\n"


def _real_frames(held):
    """How many of a new's / an advance's frames are the video's: the rest repeats the last one (the padding of a short round)."""
    n = len(held)
    while n > 1 and held[n - 1] == held[n - 2]:
        n -= 1
    return n


@pytest.mark.parametrize("driver", ["pipelined", "subpel", "bidirectional", "interpolate", "interpolate_bgr", "colorize"])
def test_video_drivers_walk_their_chains_by_the_plan(monkeypatch, driver):
    _, decode, bidirectional = _walk_drivers()[driver]
    estimate = "estimate_bidirectional_async" if bidirectional else "estimate_async"
    writes = ("new", "set_speculation", "advance", "estimate_async", "estimate_bidirectional_async", "close")
    for n_frames, in_flight, batch in WALK_GRID:
        what = "%s: n_frames %d, in_flight %d, batch %d" % (driver, n_frames, in_flight, batch)
        n_pairs = n_frames - 1
        per = max(1, min(batch, in_flight, n_pairs))
        res, log = _walk(monkeypatch, driver, n_frames, in_flight, batch)
        assert not isinstance(res, Exception), what
        assert decode(res) == [(k, k + 1) for k in range(n_pairs)], what         # result k is of frames (k, k + 1)
        chains = sorted({e[1] for e in log})
        n_ctx = len(chains)
        assert chains == list(range(n_ctx)) and sum(1 for e in log if e[0] == "new") == n_ctx, what
        handed = 0
        for e in log:
            if e[0] in ("new", "advance"):
                held = e[2]
                assert len(held) == per + (e[0] == "new"), what
                real = _real_frames(held)
                assert list(held[:real]) == list(range(held[0], held[0] + real)), what      # consecutive frames, then repeats
                handed += real
        assert handed == n_pairs + n_ctx, what                                   # every frame set once, plus one per chain
        for c in chains:
            mine = [e for e in log if e[1] == c]
            assert mine[0][0] == "new" and mine[-1] == ("close", c) and sum(1 for e in mine if e[0] == "close") == 1, what
            spec = [e for e in mine if e[0] == "set_speculation"]
            assert spec == ([("set_speculation", c, False)] if n_ctx * per > 1 else []), what
            assert not spec or mine[1] == spec[0], what
            # the reads of a round lie between its estimate and the next advance (or the close)
            state, reads = "set", 0
            for e in mine[1:]:
                if e[0] == "set_speculation":
                    continue
                if e[0] == estimate:
                    assert state == "set", what
                    state, reads = "estimated", 0
                elif e[0] in ("advance", "close"):
                    assert state == "estimated" and reads > 0, what
                    state = "set"
                else:
                    assert e[0] not in writes and state == "estimated", what
                    reads += 1
        # a read that raises in the third round: the error comes out, nothing more is enqueued and every chain is closed once
        res, log = _walk(monkeypatch, driver, n_frames, in_flight, batch, fail_round=3)
        rounds = sum(1 for e in log if e[0] == estimate)
        assert isinstance(res, RuntimeError) == (rounds >= 3), what
        made = {e[1] for e in log if e[0] == "new"}
        assert sorted(e[1] for e in log if e[0] == "close") == sorted(made), what
        if isinstance(res, RuntimeError):
            k = next(i for i, e in enumerate(log) if e[0] == "raise")
            assert all(e[0] == "close" for e in log[k + 1:]), what
