"""Long-lived contexts against the oracle: one context fed a sequence of pairs through every input path, estimates mixed with
stage calls and mode switches, planes refilled in place behind the library's back, several live contexts sharing a kernel's
LDS limit, the knobs the README calls result-neutral, and producer ordering across streams.  What a parity suite built from
fresh contexts cannot see: the state a context keeps between calls (the SAD memo, the captured graph, per-kernel attributes,
knobs read at creation).  Every field and stage grid must equal the oracle's bit for bit."""
import ctypes as C

import numpy as np
import pytest

from helpers import KNOB_CASES, gpu_schedule, oracle_schedule

pytestmark = pytest.mark.gpu


def _pair(kind, w, h, rng):
    """The content kinds of test_gpu_parity._random_case."""
    if kind == 0:                       # smooth texture + piecewise motion
        from blockbasedmotionestimation_amd.synth import synth_pair
        f1, f2, _ = synth_pair(w, h, int(rng.integers(1 << 30)), max_motion=int(rng.integers(1, 12)))
    elif kind == 1:                     # white noise, shifted by an odd amount
        f1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        f2 = np.roll(f1, (int(rng.integers(-4, 5)) * 2 + 1, int(rng.integers(-4, 5)) * 2 - 1), axis=(0, 1))
    elif kind == 2:                     # few grey levels: ties everywhere
        f1 = (rng.integers(0, 3, (h, w)) * 100).astype(np.uint8)
        f2 = (rng.integers(0, 3, (h, w)) * 100).astype(np.uint8)
    elif kind == 3:                     # flat regions next to texture
        f1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        f1[: h // 2, : w // 2] = 50
        f2 = np.roll(f1, 3, axis=1)
        f2[h // 3:, w // 3:] = 200
    else:                               # unrelated frames
        f1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        f2 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return np.ascontiguousarray(f1), np.ascontiguousarray(f2)


def _expect(oracle, f1, f2, search, block, raster=False, jacobi=False):
    omf = oracle.OracleMF(f1, f2, search, block)
    omf.set_raster_search(raster)
    omf.set_jacobi_regularizer(jacobi)
    flow = omf.calc_motion_block_matching().copy()
    omf.close()
    return flow


def _assert_same(got, exp, what):
    bad = np.argwhere((got != exp).any(-1))
    assert bad.size == 0, "%s: %d of %d pixels differ, first at %s: oracle %s gpu %s" % (
        what, len(bad), exp.shape[0] * exp.shape[1], bad[0], exp[tuple(bad[0])], got[tuple(bad[0])])


def _make_mf(bbme, monkeypatch, env, f1, f2, search, block):
    """A context created under `env` (knobs are read when a context is created); the variables are gone afterwards."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return bbme.MF(f1, f2, search, block, len(block))
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _hip():
    """The HIP runtime this process already has loaded (torch's; libbbme.so resolves to the same one)."""
    with open("/proc/self/maps") as maps:
        for line in maps:
            if "libamdhip64.so" in line:
                lib = C.CDLL(line.split()[-1])
                lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
                lib.hipMemcpy.restype = C.c_int
                lib.hipDeviceSynchronize.restype = C.c_int
                return lib
    raise RuntimeError("libamdhip64.so is not loaded")


# ---- A. one context, a sequence of different pairs, arriving by every input path ---------------------------------------
# fast: the QSAD strip kernel on every level (B 8 / 16, R <= 63); generic: k_search_generic (B = 4 on level 0, R = 72 on level 2)
GEOMETRIES = {
    "fast": (352, 256, [48, 40, 40], [16, 16, 8]),
    "generic": (320, 240, [24, 24, 160], [4, 8, 16]),
}
MODES = {
    "graph": {},                                   # the default: capture on the first estimate, replay after
    "no_graph": {"BBME_NO_GRAPH": "1"},
    "speculate_all": {"BBME_SPEC_MIN_GABS": "0"},  # every level's search speculated, the fix-up list from a changed prediction
}
ARRIVALS = ["host", "device_strided", "planes", "capi_host_pitch", "device", "host", "capi_host_pitch", "planes"]
_SEQ_CACHE = {}


def _sequence(oracle, geom):
    """8 distinct pairs of mixed content, with the oracle's field and level planes of each (computed once per geometry)."""
    if geom not in _SEQ_CACHE:
        w, h, search, block = GEOMETRIES[geom]
        rng = np.random.default_rng(4100 + len(geom))
        seq = []
        for i, arrival in enumerate(ARRIVALS):
            f1, f2 = _pair(i % 5, w, h, rng)
            omf = oracle.OracleMF(f1, f2, search, block)
            planes = [(omf.image(l, 1).copy(), omf.image(l, 2).copy()) for l in range(len(block))]
            exp = omf.calc_motion_block_matching().copy()
            omf.close()
            seq.append((arrival, f1, f2, planes, exp))
        _SEQ_CACHE[geom] = seq
    return _SEQ_CACHE[geom]


def _feed(bbme, mf, arrival, f1, f2, planes, keep):
    import torch
    from blockbasedmotionestimation_amd import _capi
    h, w = f1.shape
    if arrival == "host":
        mf.set_frames(f1, f2)
    elif arrival == "device":
        mf.set_frames_device(torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda())
    elif arrival == "device_strided":
        # views into wider allocations: row pitch w + 48, a column offset of 8
        big = torch.zeros((2, h, w + 48), dtype=torch.uint8, device="cuda")
        big[0, :, 8:8 + w] = torch.from_numpy(f1).cuda()
        big[1, :, 8:8 + w] = torch.from_numpy(f2).cuda()
        t1, t2 = big[0, :, 8:8 + w], big[1, :, 8:8 + w]
        assert t1.stride(0) == w + 48 > w
        mf.set_frames_device(t1, t2)
    elif arrival == "planes":
        for lvl, (p1, p2) in enumerate(planes):
            mf.set_level_planes(lvl, p1, p2)
    elif arrival == "capi_host_pitch":
        # bbme_set_frames_host with a host pitch wider than the frame; garbage in the bytes past each row
        pitch = w + 24
        wide = np.full((2, h, pitch), 0xA5, np.uint8)
        wide[0, :, :w] = f1
        wide[1, :, :w] = f2
        keep.append(wide)
        _capi.check(mf._lib.bbme_set_frames_host(mf._ctx, wide[0].ctypes.data, wide[1].ctypes.data, pitch))
    else:
        raise AssertionError(arrival)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_one_context_a_sequence_of_pairs(bbme, oracle, monkeypatch, geom, mode):
    """One context, 8 different pairs: every field must be the oracle's, whichever path brought the pair in and whatever the
    context computed before it."""
    w, h, search, block = GEOMETRIES[geom]
    seq = _sequence(oracle, geom)
    mf = _make_mf(bbme, monkeypatch, MODES[mode], seq[-1][1], seq[-1][2], search, block)
    keep = []
    for i, (arrival, f1, f2, planes, exp) in enumerate(seq):
        _feed(bbme, mf, arrival, f1, f2, planes, keep)
        _assert_same(mf.calcMotionBlockMatching(), exp, "%s %s pair %d (%s)" % (geom, mode, i, arrival))
    mf.close()


# ---- B. estimates mixed with stage calls and mode switches ----------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_estimates_mixed_with_stage_calls_and_mode_switches(bbme, oracle, geom):
    """estimate, the stage-by-stage schedule on new frames, estimate again; spiral -> raster -> spiral and exact -> Jacobi ->
    exact in between.  Each field against the oracle in the matching mode."""
    w, h, search, block = GEOMETRIES[geom]
    L = len(block)
    rng = np.random.default_rng(4200 + len(geom))
    pairs = [_pair(k, w, h, rng) for k in (0, 1, 3, 4, 2, 0)]
    mf = bbme.MF(pairs[0][0], pairs[0][1], search, block, L)
    steps = [  # (pair, raster, jacobi, how)
        (0, False, False, "estimate"),
        (1, False, False, "stages"),
        (2, True, False, "estimate"),
        (3, True, False, "stages"),
        (4, False, False, "estimate"),
        (5, False, True, "estimate"),
        (0, False, False, "estimate"),
        (1, False, True, "estimate"),
        (2, False, False, "stages"),
        (3, False, False, "estimate"),
    ]
    for i, (p, raster, jacobi, how) in enumerate(steps):
        f1, f2 = pairs[p]
        mf.set_search_mode(raster)
        mf.set_regularizer_mode(jacobi)
        mf.set_frames(f1, f2)
        if how == "estimate":
            got = mf.calcMotionBlockMatching()
        else:
            got = gpu_schedule(mf, L, block)
        exp = _expect(oracle, f1, f2, search, block, raster=raster, jacobi=jacobi)
        _assert_same(got, exp, "%s step %d: pair %d raster=%s jacobi=%s by %s" % (geom, i, p, raster, jacobi, how))
    mf.close()


# ---- C. level planes refilled in place through bbme_level_planes_device -----------------------------------------------------
def _check_sweeps(mf, omf, B, what, nsweeps=None, lookups=None):
    """The sweeps of a one-level schedule from the grid both sides hold now (regularize_MVs at B, B/2, ... 2, lambda
    multipliers 1 and 2), each grid compared; nsweeps: stop after that many; lookups: a list that collects each sweep's SAD
    memo look-ups (sweep_stats [9])."""
    b, lam, n = B, float(B // 2), 0
    while b > 1:
        for mult in (1, 2):
            omf.set_block_size(0, b)
            omf.set_lambda(0, lam)
            omf.regularize_mvs(0, mult)
            mf.stage_regularize(0, b, mult)
            got, exp = mf.stage_get_mvs(0, b).astype(np.int32), omf.block_mvs(0, b)
            assert np.array_equal(got, exp), "%s: sweep at b=%d mult %d: %d of %d blocks differ" % (
                what, b, mult, int((got != exp).any(-1).sum()), exp.shape[0] * exp.shape[1])
            if lookups is not None:
                lookups.append(mf.sweep_stats()[9])
            n += 1
            if nsweeps is not None and n >= nsweeps:
                return
        omf.divide_blocks(0)
        b >>= 1
        lam *= 2


def _flood_grid(rows, cols, u, v, rng):
    """u everywhere, v at three seed blocks and a few obstacles with other vectors: on frames that move by v, v floods the grid
    in one sweep, and pass 1 memoises the SADs of every non-uniform neighbourhood on the way (test_sad_memo_hits_and_misses)."""
    g = np.empty((rows, cols, 2), np.int16)
    g[...] = u
    for r, c in ((0, 0), (3, 9), (7, 2)):
        g[r, c] = v
    for _ in range(6):
        g[int(rng.integers(0, rows)), int(rng.integers(0, cols))] = (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
    return g


@pytest.mark.parametrize("b,first,env", [
    (16, "search", {}),
    (32, "search", {}),
    (16, "set_mvs", {}),
    (32, "set_mvs", {}),
    (8, "search", {"BBME_MEMO_MIN_B": "8"}),
    (8, "set_mvs", {"BBME_MEMO_MIN_B": "8"}),
], ids=["b16_search", "b32_search", "b16_set_mvs", "b32_set_mvs", "b8_memo_search", "b8_memo_set_mvs"])
def test_in_place_plane_refill_between_stage_sequences(bbme, oracle, monkeypatch, b, first, env):
    """bbme.h lets a caller fill a level's planes in place through the pointers bbme_level_planes_device returns, without
    telling the library.  The SAD memo of the regulariser (b >= 16 by default) holds SADs of the planes it was filled from:
    a stage sequence started after the refill (stage_search or stage_set_mvs, as bbme.h requires) must not take them.  The
    level's search (or a given grid), then the first sweep on planes A; refill with planes B by a raw hipMemcpy; the whole
    level again on B, every grid against the oracle on B; then a full estimate on B.
    set_mvs: the same flood grid before and after the refill, so that the first sweep on B looks up exactly the slots the
    sweep on A filled.  A moves by v, B by u: SADs taken from A would flood v over B."""
    rng = np.random.default_rng(4300 + b)
    rows, cols = 12, 18
    w, h = cols * b, rows * b
    search, block = [b + 16], [b]
    v, u = (2, -1), (0, 0)
    if first == "search":                                          # two pairs of smooth content with piecewise motion
        (a1, a2), (b1, b2) = _pair(0, w, h, rng), _pair(0, w, h, rng)
    else:
        a1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        a2 = np.roll(a1, (v[1], v[0]), axis=(0, 1))
        b1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        b2 = np.roll(b1, (u[1], u[0]), axis=(0, 1))
    grid = _flood_grid(rows, cols, u, v, rng)
    omf_a = oracle.OracleMF(a1, a2, search, block)
    omf_b = oracle.OracleMF(b1, b2, search, block)
    mf = _make_mf(bbme, monkeypatch, dict({"BBME_MEMO": "1"}, **env), a1, a2, search, block)
    d1, d2 = mf.level_planes_device(0)                             # held from here on
    pw, ph, _, _ = mf.level_geometry(0)
    assert omf_b.image(0, 1).shape == (ph, pw)
    mf.set_level_planes(0, omf_a.image(0, 1), omf_a.image(0, 2))

    def start(omf, what):
        if first == "search":
            omf.calc_level_bm(0)
            mf.stage_search(0)
        else:
            omf.flow(0)[...] = 0
            omf.flow(0)[::b, ::b, :] = grid
            mf.stage_set_mvs(0, b, grid)
        got, exp = mf.stage_get_mvs(0, b).astype(np.int32), omf.block_mvs(0, b)
        assert np.array_equal(got, exp), "%s: the starting grid differs" % what

    start(omf_a, "planes A")
    filled = []
    _check_sweeps(mf, omf_a, b, "planes A", nsweeps=1, lookups=filled)   # the first sweep at b fills the memo from planes A
    hip = _hip()
    for dst, src in ((d1, omf_b.image(0, 1)), (d2, omf_b.image(0, 2))):
        src = np.ascontiguousarray(src)
        assert hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src.ctypes.data), src.nbytes, 1) == 0     # hipMemcpyHostToDevice
    assert hip.hipDeviceSynchronize() == 0
    start(omf_b, "planes B")
    looked = []
    _check_sweeps(mf, omf_b, b, "b=%d %s: planes B refilled in place" % (b, first), lookups=looked)
    if first == "set_mvs":
        # the premise of the flood variant: the memo served the sweep on A and the first sweep on B
        assert filled[0] > 0 and looked[0] > 0, (filled, looked)
    mf.stage_expand()
    omf_b.set_block_size(0, 2)
    omf_b.copy_to_all_pixels(0)
    _assert_same(mf.get_flow(), omf_b.flow(0), "b=%d: expanded field after the refill" % b)
    _assert_same(mf.calcMotionBlockMatching(), _expect(oracle, b1, b2, search, block), "b=%d: estimate after the refill" % b)
    mf.close()
    omf_a.close()
    omf_b.close()


# ---- D. live contexts that share a kernel's LDS limit ----------------------------------------------------------------------
@pytest.mark.parametrize("B,big,small", [(16, 270, 236), (32, 286, 232)], ids=["b16_r127_r110", "b32_r127_r100"])
def test_live_contexts_sharing_a_search_kernel(bbme, oracle, B, big, small):
    """hipFuncAttributeMaxDynamicSharedMemorySize belongs to k_search_generic<B>, not to a context.  A context needing a large
    window (R = 127: 74 776 B at B = 16, 84 536 B at B = 32), then a second live one with a smaller window that still needs more
    than 48 KB: the second must not lower the first's limit.  R = 127, the smaller, R = 127 again, each against the oracle."""
    rng = np.random.default_rng(4400 + B)
    f1, f2 = _pair(1, 384, 384, rng)
    exp_big = _expect(oracle, f1, f2, [big], [B])
    exp_small = _expect(oracle, f1, f2, [small], [B])
    mf_big = bbme.MF(f1, f2, [big], [B], 1)
    mf_small = bbme.MF(f1, f2, [small], [B], 1)
    for mf, exp, what in ((mf_big, exp_big, "R=127"), (mf_small, exp_small, "smaller window"), (mf_big, exp_big, "R=127 again")):
        _assert_same(mf.calcMotionBlockMatching(), exp, "B=%d %s" % (B, what))
    mf_small.close()
    mf_big.close()


@pytest.mark.parametrize("per_cu", ["2", "1", "24,1"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_speculative_search_lds_floor(bbme, oracle, monkeypatch, geom, per_cu):
    """BBME_SPEC_WGS_PER_CU pads every speculative search workgroup to 120 KB / n of LDS (61 440 B at 2, 122 880 B at 1) --
    above what a kernel gets by default, on the strip kernel as on the generic one.  With speculation on every level the
    field must still be the oracle's, and no launch may be refused."""
    w, h, search, block = GEOMETRIES[geom]
    arrival, f1, f2, planes, exp = _sequence(oracle, geom)[1]
    mf = _make_mf(bbme, monkeypatch, {"BBME_SPEC_WGS_PER_CU": per_cu, "BBME_SPEC_MIN_GABS": "0"}, f1, f2, search, block)
    _assert_same(mf.calcMotionBlockMatching(), exp, "%s per_cu=%s" % (geom, per_cu))
    _assert_same(mf.calcMotionBlockMatching(), exp, "%s per_cu=%s, replay" % (geom, per_cu))
    mf.close()


# ---- E. the knobs the README calls result-neutral --------------------------------------------------------------------------
@pytest.mark.parametrize("name,env,cases", KNOB_CASES, ids=[k[0] for k in KNOB_CASES])
def test_result_neutral_knobs(bbme, oracle, monkeypatch, name, env, cases):
    """Every knob of README's table "changes no result": a context created under it returns the oracle's field, twice (the
    second from the graph replay).  The knobs are read when a context is created, so one process can test them all."""
    rng = np.random.default_rng(4500 + len(name))
    for w, h, search, block, kind in cases:
        f1, f2 = _pair(kind, w, h, rng)
        exp = _expect(oracle, f1, f2, search, block)
        mf = _make_mf(bbme, monkeypatch, env, f1, f2, search, block)
        _assert_same(mf.calcMotionBlockMatching(), exp, "%s %s" % (name, (w, h, search, block)))
        _assert_same(mf.calcMotionBlockMatching(), exp, "%s %s, replay" % (name, (w, h, search, block)))
        mf.close()


def test_relax_rule_is_read_per_context(bbme, oracle, monkeypatch):
    """BBME_RELAX_RULE reaches the context it was set for, in a process that created contexts before: with relaxation launches
    on every sweep, the tile kernel settles most changes and the solver re-evaluates fewer blocks over the schedule
    (sweep_stats [4]) than without; every stage grid against the oracle either way."""
    rng = np.random.default_rng(4600)
    f1, f2 = _pair(4, 256, 192, rng)
    search, block = [40, 40], [8, 8]
    evaluated = {}
    for rule in ("300000,2,1,0", "0,64,2,2", "300000,2,1,0"):
        omf = oracle.OracleMF(f1, f2, search, block)
        mf = _make_mf(bbme, monkeypatch, {"BBME_RELAX_RULE": rule}, f1, f2, search, block)
        for lvl in range(len(block)):
            mf.set_level_planes(lvl, omf.image(lvl, 1), omf.image(lvl, 2))
        exp, got = [], []
        oflow = oracle_schedule(omf, len(block), lambda *a: exp.append(a))
        total = [0]

        def on_stage(name, lvl, b, mv):
            got.append((name, lvl, b, mv))
            if name.startswith("sweep"):
                total[0] += mf.sweep_stats()[4]

        gflow = gpu_schedule(mf, len(block), block, on_stage)
        for (en, el, eb, ev), (gn, gl, gb, gv) in zip(exp, got):
            assert (en, el, eb) == (gn, gl, gb) and np.array_equal(ev, gv), (rule, en, el, eb)
        assert np.array_equal(oflow, gflow), rule
        evaluated.setdefault(rule, []).append(total[0])
        mf.close()
        omf.close()
    assert max(evaluated["0,64,2,2"]) < min(evaluated["300000,2,1,0"]), evaluated


# ---- F. producer ordering -------------------------------------------------------------------------------------------------
def _delay(stream):
    """Keep `stream` busy for a while before what is queued on it next."""
    import torch
    with torch.cuda.stream(stream):
        try:
            torch.cuda._sleep(100_000_000)
        except (AttributeError, RuntimeError):
            x = torch.randn(2048, 2048, device="cuda")
            for _ in range(40):
                x = x @ x
                x = x / x.abs().max()


def test_wait_for_stream_orders_frames_written_on_a_side_stream(bbme, oracle):
    """The next frames are written into the device tensors on a torch side stream behind a delay; bbme_wait_for_stream on that
    stream, then bbme_set_frames_device and an estimate: the field must be the oracle's for the NEW frames."""
    import torch
    from blockbasedmotionestimation_amd import _capi
    w, h, search, block = GEOMETRIES["fast"]
    rng = np.random.default_rng(4700)
    (f1, f2), (g1, g2) = _pair(0, w, h, rng), _pair(1, w, h, rng)
    t1, t2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    n1, n2 = torch.from_numpy(g1).cuda(), torch.from_numpy(g2).cuda()
    torch.cuda.synchronize()
    mf = bbme.MF(t1, t2, search, block, len(block), frames_on_device=True)
    _assert_same(mf.calcMotionBlockMatching(), _expect(oracle, f1, f2, search, block), "first pair")
    side = torch.cuda.Stream()
    _delay(side)
    with torch.cuda.stream(side):
        t1.copy_(n1)
        t2.copy_(n2)
    _capi.check(mf._lib.bbme_wait_for_stream(mf._ctx, C.c_void_p(side.cuda_stream)))
    _capi.check(mf._lib.bbme_set_frames_device(mf._ctx, t1.data_ptr(), t2.data_ptr(), t1.stride(0)))
    _assert_same(mf.calcMotionBlockMatching(), _expect(oracle, g1, g2, search, block), "frames written on the side stream")
    side.synchronize()
    mf.close()


def test_set_stream_between_graph_replays(bbme, oracle, monkeypatch):
    """With speculation on every level: estimate (graph captured on the context's own stream), then set_stream onto a torch
    stream and estimate new pairs there, then back to a stream of the context's own."""
    import torch
    w, h, search, block = GEOMETRIES["fast"]
    seq = _sequence(oracle, "fast")
    mf = _make_mf(bbme, monkeypatch, {"BBME_SPEC_MIN_GABS": "0"}, seq[0][1], seq[0][2], search, block)
    _assert_same(mf.calcMotionBlockMatching(), seq[0][4], "own stream")
    s = torch.cuda.Stream()
    mf.set_stream(s.cuda_stream)
    for i in (1, 2):
        mf.set_frames(seq[i][1], seq[i][2])
        _assert_same(mf.calcMotionBlockMatching(), seq[i][4], "torch stream, pair %d" % i)
    mf.set_stream(0)
    mf.set_frames(seq[3][1], seq[3][2])
    _assert_same(mf.calcMotionBlockMatching(), seq[3][4], "back on an own stream")
    mf.close()


# ---- F. the pair setters on a batch: one slot numbering for the planes, the upload buffer and the colour store ----------
# 48 x 40 frames are padded to 64 x 64 / 32 x 32: at both levels the image-2 planes of three pairs start where no multiple of
# the plane stride lies, and the planes, the upload buffer and the colour store each keep frame `which` of pair p in slot
# which * 3 + p.  A wrong step or slot number puts a frame of pair 1 into a plane of pair 0 or 2, or takes it from theirs.
SMALL = ([30, 30], [16, 16])
PAIR_SETTERS = ["grey_host", "grey_device", "x4_host", "x4_device", "bgr_host", "bgr_device"]
SHIFTS = {"x4": [(1, -1), (-1, 1), (1, 1), (0, -1)]}        # source pixels: four times as far in the frame
SHIFTS["grey"] = SHIFTS["bgr"] = [(3, -2), (-1, 4), (2, 2), (-3, -1)]


def _small_pair(fmt, i):
    """Content i of a format: noise and the same noise moved by SHIFTS[fmt][i]; x4: sources of a quarter of the frame; bgr:
    three pointwise maps of the grey pair."""
    w, h = (12, 10) if fmt == "x4" else (48, 40)
    f1 = np.random.default_rng(5200 + i).integers(0, 256, (h, w), dtype=np.uint8)
    f2 = np.roll(f1, SHIFTS[fmt][i], axis=(0, 1))
    if fmt == "bgr":
        f1, f2 = (np.stack([v, 255 - v, (v.astype(np.int32) * 3 // 4 + 30).astype(np.uint8)], -1) for v in (f1, f2))
    return np.ascontiguousarray(f1), np.ascontiguousarray(f2)


def _call_pair_setter(lib, ctx, kind, pair, f1, f2, alive):
    """The C-ABI pair setter of `kind` on packed host frames, or on frames in HBM whose rows are 13 bytes further apart."""
    import torch
    from blockbasedmotionestimation_amd import _capi
    fmt, where = kind.split("_")
    setter = getattr(lib, {"grey": "bbme_set_frames_%s_pair", "x4": "bbme_set_frames_%s_x4", "bgr": "bbme_set_frames_%s_bgr"}[fmt] % where)
    h, row = f1.shape[0], f1[0].size
    if where == "host":
        _capi.check(setter(ctx, pair, f1.ctypes.data, f2.ctypes.data, row))
        return
    wide = torch.full((2, h, row + 13), 0xAA, dtype=torch.uint8, device="cuda")
    wide[0, :, :row] = torch.from_numpy(f1.reshape(h, row)).cuda()
    wide[1, :, :row] = torch.from_numpy(f2.reshape(h, row)).cuda()
    torch.cuda.synchronize()
    _capi.check(setter(ctx, pair, wide[0].data_ptr(), wide[1].data_ptr(), row + 13))
    alive.append(wide)                                     # until the context's stream has read it


def _stored_colour(mf, pair, shape):
    """The two frames the colour store holds for `pair` (packed, pitch 3 W)."""
    mf.synchronize()
    out = []
    for ptr in mf.bgr_frames_device_ptrs(pair):
        buf = np.empty(shape, np.uint8)
        assert _hip().hipMemcpy(buf.ctypes.data, ptr, buf.nbytes, 2) == 0
        out.append(buf)
    return out


@pytest.mark.parametrize("kind", PAIR_SETTERS)
def test_resetting_one_pair_of_a_batch_through_every_pair_setter(bbme, kind):
    """A batch of three pairs, every pair set through the setter under test, then pair 1 alone set again to other content: the
    cells of pairs 0 and 2 stay what they were, every pair's cells are those of a single context on the same frames, and the
    colour store holds every pair's frames in its own slots."""
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    fmt = kind.split("_")[0]
    up = 4 if fmt == "x4" else 1
    search, block = SMALL
    content = [_small_pair(fmt, i) for i in range(4)]          # pairs 0, 1, 2, and what pair 1 is set to again
    singles = []
    for f1, f2 in content:
        mf = bbme.MF(f1, f2, search, block, upsample=up)
        mf.estimate_async()
        singles.append(mf.get_cells())
        mf.close()
    assert all(not np.array_equal(singles[i], singles[j]) for i in range(4) for j in range(i))     # the test can tell them apart
    z = np.zeros(content[0][0].shape[:2], np.uint8)
    mb = bbme.MFBatch([(z, z)] * 3, search, block, upsample=up)
    assert (mb.padded_width, mb.padded_height) == (64, 64)
    alive = []
    for p in range(3):
        _call_pair_setter(lib, mb._ctx, kind, p, *content[p], alive)
    mb.estimate_async()
    before = [mb.get_pair_cells(p) for p in range(3)]
    for p in range(3):
        assert np.array_equal(before[p], singles[p]), "pair %d" % p
        if fmt == "bgr":
            assert all(np.array_equal(a, b) for a, b in zip(_stored_colour(mb, p, content[p][0].shape), content[p])), "colour of pair %d" % p
    _call_pair_setter(lib, mb._ctx, kind, 1, *content[3], alive)
    mb.estimate_async()
    for p, exp in enumerate((singles[0], singles[3], singles[2])):
        assert np.array_equal(mb.get_pair_cells(p), exp), "pair %d after pair 1 was set again" % p
    assert np.array_equal(mb.get_pair_cells(0), before[0]) and np.array_equal(mb.get_pair_cells(2), before[2])
    if fmt == "bgr":
        now = (content[0], content[3], content[2])
        for p in range(3):
            assert all(np.array_equal(a, b) for a, b in zip(_stored_colour(mb, p, now[p][0].shape), now[p])), "colour of pair %d" % p
        # a grey setter of pair 1 withdraws the colour of pair 1 only
        mb.set_pair(1, content[1][0][..., 0], content[1][1][..., 0])
        with pytest.raises(bbme.BbmeError) as e:
            mb.bgr_frames_device_ptrs(1)
        assert e.value.status == _capi.ERR_STATE
        for p in (0, 2):
            assert all(np.array_equal(a, b) for a, b in zip(_stored_colour(mb, p, now[p][0].shape), now[p])), "colour of pair %d" % p
    mb.close()


def test_a_batch_of_64_pairs_set_last_pair_first(bbme):
    """BBME_MAX_BATCH pairs are 128 frame slots, one flag each (where a 64-bit word of pairs used to end): pair 63 set first and
    pair 0 last, an estimate refused until every pair has frames.  8 x 8 frames in two levels of 2 x 2 blocks, +-1: the narrowest
    levels a context takes (test_gpu_parity).  The chain's counterpart is test_gpu_chain.test_a_chain_of_64_pairs_has_65_slots."""
    from blockbasedmotionestimation_amd import _capi
    lib = _capi.lib()
    w, h, search, block = 8, 8, [4, 4], [2, 2]
    rng = np.random.default_rng(5300)
    pairs = []
    for p in range(64):
        f1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        pairs.append((f1, np.ascontiguousarray(np.roll(f1, (p % 3 - 1, p // 3 % 3 - 1), axis=(0, 1)))))
    params = _capi.make_params(search, block)
    ctx = C.c_void_p()
    assert lib.bbme_create_batch(C.byref(params), w, h, 0, 65, C.byref(ctx)) == _capi.ERR_INVALID
    _capi.check(lib.bbme_create_batch(C.byref(params), w, h, 0, 64, C.byref(ctx)))
    for p in [63] + list(range(1, 63)) + [0]:
        assert lib.bbme_estimate(ctx) == _capi.ERR_STATE, "before pair %d is set" % p
        _capi.check(lib.bbme_set_frames_host_pair(ctx, p, pairs[p][0].ctypes.data, pairs[p][1].ctypes.data, w))
    _capi.check(lib.bbme_estimate(ctx))
    for p in (0, 31, 63):
        got = np.empty((h // 2, w // 2, 2), np.int16)
        _capi.check(lib.bbme_get_cells_host_pair(ctx, p, got.ctypes.data))
        mf = bbme.MF(pairs[p][0], pairs[p][1], search, block)
        mf.estimate_async()
        assert np.array_equal(got, mf.get_cells()), "pair %d" % p
        mf.close()
    _capi.check(lib.bbme_destroy(ctx))


# ---- one staging area per context serves every host getter, in any order -----------------------------------------------------
# name -> the getter on pair 1 of a bidirectional batch; in the order of the bytes they stage (96 x 72 frames, 128 x 128 planes)
_STAGED_GETTERS = [
    ("sub4", lambda mf: mf.get_pair_subsampled_flow(1, 4)),                     # 3 456 bytes
    ("mask", lambda mf: mf.consistency("backward", 1, pair=1)),                 # 4 096
    ("mc_level1", lambda mf: mf.get_pair_motion_compensated(1, level=1, block=4, fill=9)),
    ("mc_level0", lambda mf: mf.get_pair_motion_compensated(1, level=0, block=2, fill=9)),      # 16 384
    ("interpolated", lambda mf: mf.get_pair_interpolated(1, 1, 3)),
    ("filtered", lambda mf: mf.get_frame_filtered(1, 0, 64)),
    ("subpel_cells", lambda mf: mf.get_pair_subpel_cells(1)),
    ("colour", lambda mf: (mf.get_pair_flow_color(1, 1), np.array(mf.last_color_range, np.float32))),      # 20 736 + the ranges
    ("interpolated_bgr", lambda mf: mf.interpolate_bgr(1, 3, pair=1)),
    ("filtered_bgr", lambda mf: mf.get_frame_filtered_bgr(1, 0, 64)),
    ("sub1", lambda mf: mf.get_pair_subsampled_flow(1, 1)),                     # 55 296
    ("subpel_flow", lambda mf: mf.get_pair_subpel_flow(1)),                     # 55 296 + 16 384 of cells behind them
]
_staged_cache = {}


def _staged_batch(bbme):
    from test_gpu_bgr import VIDEO_PARAMS, colour_video
    frames = [np.ascontiguousarray(f[:72, :96]) for f in colour_video(bbme)[:3]]
    mf = bbme.MFBatch([(frames[0], frames[1]), (frames[1], frames[2])], *VIDEO_PARAMS)
    mf.estimate_bidirectional_async()
    return mf


def _staged_x4_batch(bbme):
    video = bbme.synth_video(48, 36, 3, 77, max_motion=2)
    mf = bbme.MFBatch([(video[0], video[1]), (video[1], video[2])], [30, 30], [16, 16], upsample=4)
    mf.estimate_bidirectional_async()
    return mf


def _staged_reference(bbme):
    """Every getter's result as the FIRST call on a fresh context (its staging area still empty); made once, never changed."""
    if not _staged_cache:
        for name, get in _STAGED_GETTERS:
            mf = _staged_batch(bbme)
            _staged_cache[name] = get(mf)
            mf.close()
        for name, get in (("x4_subpel_flow", lambda mf: mf.get_pair_subpel_flow(1)),
                          ("x4_subpel_cells", lambda mf: mf.get_pair_subpel_cells(1))):
            mf = _staged_x4_batch(bbme)
            _staged_cache[name] = get(mf)
            mf.close()
    return _staged_cache


def _same_bytes(got, exp):
    got, exp = (x if isinstance(x, tuple) else (x,) for x in (got, exp))
    return len(got) == len(exp) and all(g.dtype == e.dtype and g.shape == e.shape and g.tobytes() == e.tobytes() for g, e in zip(got, exp))


@pytest.mark.parametrize("order", ["ascending", "descending", "subpel_flow_first"])
def test_one_staging_area_serves_every_host_getter_in_any_order(bbme, order):
    ref = _staged_reference(bbme)
    getters = {"ascending": _STAGED_GETTERS, "descending": _STAGED_GETTERS[::-1],
               "subpel_flow_first": _STAGED_GETTERS[-1:] + _STAGED_GETTERS[:-1]}[order]
    mf = _staged_batch(bbme)
    try:
        for name, get in getters + getters[:2]:                      # and the first two again, behind everything else
            assert _same_bytes(get(mf), ref[name]), "%s order: %s differs from a fresh context's" % (order, name)
    finally:
        mf.close()
    assert ref["sub4"].shape == (18, 24, 2) and ref["subpel_flow"].shape == (72, 96, 2) and ref["colour"][1].shape == (5,)
    assert np.abs(ref["subpel_flow"]).max() > 0 and len(np.unique(ref["colour"][0])) > 8      # results, not blank buffers


def test_subpel_field_and_cells_share_the_area_on_an_upsampling_context(bbme):
    """upsample=4: the field (48 x 36 x 2 floats) is not the size of the cells it is expanded from (the x4 planes' 2x2 cells),
    so the cells' region does not start where a cells-only download puts them."""
    ref = _staged_reference(bbme)
    mf = _staged_x4_batch(bbme)
    try:
        assert ref["x4_subpel_flow"].shape == (36, 48, 2) and ref["x4_subpel_cells"].shape == mf.cells_shape + (2,)
        assert ref["x4_subpel_flow"].nbytes != ref["x4_subpel_cells"].nbytes
        for name, get in (("x4_subpel_flow", mf.get_pair_subpel_flow), ("x4_subpel_cells", mf.get_pair_subpel_cells),
                          ("x4_subpel_flow", mf.get_pair_subpel_flow)):
            assert _same_bytes(get(1), ref[name]), name
    finally:
        mf.close()
