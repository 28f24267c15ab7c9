"""Colour coding of the motion field on the GPU (include/bbme.h, "COLOUR RULE"): k_color_range / k_color_image give, bit for
bit, the host mirror bbme.color_cells -- image and the five range floats -- on crafted grids (every integer vector with |dx|,
|dy| <= 40 embedded in random cells, the axes, all zeros), at scale 1, 3, 4, with and without a fixed maxmotion; through every
store path (row tails, caller pitches and offsets that are no multiple of 4, odd pads, guard bytes); after real estimates
(forward, backward, an upsample=4 context at scale 4) they also agree with Flow::MotionToColor of the downloaded field within the
atan2 cap of tests/test_host_cpu.py, taken over DISTINCT vectors; batches and chains equal single contexts; the calls change no
context state and refuse bad arguments; bbme_cli --backward-color writes the same pixels.

Rows of more than 1024 sampled cells (frames 2100, 2098 and 1030 pixels wide, 8 to 32 high) reach what the 200 x 170 contexts
cannot: the second, third and fourth cell a lane of k_color_range folds and its second workgroup per row.  There one cell at a time
carries the only large vector, so the range -- and with it every pixel of the image -- is right only if that lane-iteration of that
tile is; vectors over the whole int16 range with normalising radii down to the smallest normal float and up to 3e38; batches and
chains whose extreme lies beyond column 1024 in one pair only; the image buffer growing from call to call.

Contexts are 200 x 170 frames (padded 208 x 176: an even pad_x, an odd pad_y, 104 x 88 cells, room for the 81 x 81 block) with
blocks of 8 and search windows of 4 on two levels (the centre candidate only: the cheapest estimate), and, so that the real
estimates also carry motion, the same with search windows of 16."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import _write_pgm
from test_flow_color_cpu import (EXTREME_MAXMOTIONS, all_vectors_grid, assert_within_atan2_cap, axes_grid, full_range_grid,
                                 np_color_cells, subsampled_field)

pytestmark = pytest.mark.gpu

W, H = 200, 170
CHEAP = ([4, 4], [8, 8])                                   # search window < block: the centre candidate only
MOVING = ([16, 16], [8, 8])                                # search range 4
FIXED = 7.5                                                # drives part of the |d| <= 40 block through rad > 1 at scale 4
_FRAMES = {}


def _pair(bbme, w=W, h=H, seed=31, max_motion=3):
    key = (w, h, seed, max_motion)
    if key not in _FRAMES:
        _FRAMES[key] = bbme.synth_pair(w, h, seed, max_motion=max_motion)[:2]
    return _FRAMES[key]


def _crafted(mf, kind, seed=0):
    """(CH, CW, 2) int16 cells of the context's geometry."""
    ch, cw = mf.cells_shape
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((ch, cw, 2), np.int16)
    g = rng.integers(-55, 56, (ch, cw, 2)).astype(np.int16)
    block = all_vectors_grid() if kind == "all" else axes_grid()
    bh, bw = block.shape[:2]
    y0, x0 = (mf.padding_y >> 1) + 2, (mf.padding_x >> 1) + 7
    assert y0 + bh <= ch and x0 + bw <= cw
    g[y0:y0 + bh, x0:x0 + bw] = block
    return g


def _host(bbme, mf, cells, scale, maxmotion):
    return bbme.color_cells(cells, mf.orig_width, mf.orig_height, mf.padding_x, mf.padding_y, scale, maxmotion)


def _device(mf, cells, scale, maxmotion, want=("out", "range"), pitch_extra=0, offset=0, stream=None):
    """cells_color_device on a host grid -> (image or None, range tuple or None).  The image lies `offset` bytes into rows that
    are pitch_extra bytes longer than packed, between two guard rows; every byte around it must stay as it was."""
    import torch
    rows, cols, _ = mf.color_shape(scale)
    pitch = 3 * cols + pitch_extra
    assert offset <= pitch_extra
    t = torch.from_numpy(np.ascontiguousarray(cells)).cuda()
    buf = torch.full(((rows + 2) * pitch,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.as_strided(buf, (rows, cols, 3), (pitch, 3, 1), pitch + offset) if "out" in want else None
    rng = torch.full((7,), -7.0, dtype=torch.float32, device="cuda") if "range" in want else None
    torch.cuda.synchronize()
    mf.cells_color_device(t, out=out, range=None if rng is None else rng[1:6], scale=scale, maxmotion=maxmotion,
                          hip_stream_handle=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    else:
        mf.synchronize()
    img = None
    if out is not None:
        host = buf.cpu().numpy().reshape(rows + 2, pitch)
        img = host[1:-1, offset:offset + 3 * cols].reshape(rows, cols, 3).copy()
        host[1:-1, offset:offset + 3 * cols] = 0xA5
        assert (host == 0xA5).all(), "bytes outside the image were written"
    else:
        assert bool((buf == 0xA5).all())
    r = None
    if rng is not None:
        r = rng.cpu().numpy()
        assert r[0] == -7.0 and r[6] == -7.0
        r = tuple(float(v) for v in r[1:6])
    return img, r


def _assert_device_equals_host(bbme, mf, cells, scale, maxmotion, what, **kw):
    img, r = _device(mf, cells, scale, maxmotion, **kw)
    exp, exp_range = _host(bbme, mf, cells, scale, maxmotion)
    assert r is None or r == exp_range, (what, scale, maxmotion, r, exp_range)
    if img is not None and not np.array_equal(img, exp):
        bad = np.argwhere((img != exp).any(-1))
        y, x = bad[0]
        cell = cells[(mf.padding_y + scale * y) >> 1, (mf.padding_x + scale * x) >> 1]
        raise AssertionError("%s scale %d maxmotion %g: %d pixels differ, first (%d, %d) vector %s: device %s host %s"
                             % (what, scale, maxmotion, len(bad), x, y, tuple(cell), img[y, x], exp[y, x]))


@pytest.mark.parametrize("kind", ["all", "axes", "zero"])
def test_cells_color_device_on_crafted_grids(bbme, kind):
    f1, f2 = _pair(bbme)
    mf = bbme.MF(f1, f2, *CHEAP)
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == (208, 176, 4, 3)
    cells = _crafted(mf, kind)
    for scale in (1, 3, 4):
        for maxmotion in (-1.0, FIXED):
            _assert_device_equals_host(bbme, mf, cells, scale, maxmotion, kind)
    if kind == "zero":
        img, r = _device(mf, cells, 1, -1.0)
        assert r == (0.0,) * 5 and (img == 255).all()
    mf.close()


@pytest.mark.parametrize("w,h", [(200, 170), (202, 172), (198, 170)])
def test_store_paths(bbme, w, h):
    f1, f2 = _pair(bbme, w, h)
    mf = bbme.MF(f1, f2, *CHEAP)
    if (w, h) == (200, 170):
        rows, cols, _ = mf.color_shape(3)
        assert cols % 4 == 3 and rows % 2 == 1                # 67 x 57: a row tail of 3 pixels, an odd number of rows
    if w != 200:
        assert mf.padding_x % 2 == 1                          # a cell straddles the frame's first column at scale 1
    cells = _crafted(mf, "all", seed=w)
    for scale in (1, 3, 4):
        for extra, offset in ((0, 0), (5, 1), (6, 2), (7, 3), (9, 0)):      # pitches 3 cols + extra: every residue mod 4 over the cases
            _assert_device_equals_host(bbme, mf, cells, scale, FIXED if extra == 6 else -1.0, "pitch + %d, offset %d" % (extra, offset),
                                       pitch_extra=extra, offset=offset, want=("out", "range") if extra != 7 else ("out",))
    _assert_device_equals_host(bbme, mf, cells, 3, -1.0, "range only", want=("range",))
    _assert_device_equals_host(bbme, mf, cells, 3, FIXED, "image only, no range pass", want=("out",), pitch_extra=5, offset=1)
    _assert_device_equals_host(bbme, mf, cells, 1, -1.0, "image only", want=("out",))
    _assert_device_equals_host(bbme, mf, cells, 2, -1.0, "scale 2", pitch_extra=3, offset=3)
    _assert_device_equals_host(bbme, mf, cells, 64, -1.0, "scale 64", pitch_extra=1, offset=1)
    _assert_device_equals_host(bbme, mf, cells, 1000, -1.0, "one pixel", pitch_extra=2, offset=1)
    mf.close()


# ---- rows of more than 1024 sampled cells: every lane-iteration and both tiles of k_color_range ------------------------------

# (frame, search, block) -> (padded width, padded height, pad_x, pad_y).  A search window <= the block is the centre candidate only
WIDE = {"2100x8": ((2100, 8, [4], [4]), (2100, 8, 0, 0)),         # 1050 sampled cells per row at scale 1 and 2: two range tiles
        "2098x16": ((2098, 16, [8], [8]), (2104, 16, 3, 0)),      # odd pad_x: a cell straddles column 0, in every one of 17 image tiles
        "1030x8": ((1030, 8, [4], [4]), (1032, 8, 1, 0))}         # 516 cells per row: lane-iterations 0 .. 2 of one tile
PROBE_COLUMNS = (255, 256, 511, 512, 767, 768, 1023, 1024)        # both sides of every lane-iteration's and of the tile's boundary
PROBE_VECTORS = ((300, 200), (-300, -200))


def _zero_mf(bbme, w, h, search, block, expect):
    z = np.zeros((h, w), np.uint8)
    assert bbme.plan_padding(w, h, search, block) == expect
    mf = bbme.MF(z, z, search, block)
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == expect
    return mf


def _sampled(mf, scale):
    """(ncx, ncy): the sampled cells per row and the rows of them, as the range pass counts them."""
    px, py, w, h = mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height
    if scale == 1:
        return ((px + w - 1) >> 1) - (px >> 1) + 1, ((py + h - 1) >> 1) - (py >> 1) + 1
    return -(-w // scale), -(-h // scale)


def _sampled_cell(mf, scale, i, j):
    """(row, column) of the one cell that sampled column i of sampled row j reads."""
    px, py = mf.padding_x, mf.padding_y
    if scale == 1:
        return (py >> 1) + j, (px >> 1) + i
    return (py + scale * j) >> 1, (px + scale * i) >> 1


def _assert_device_equals_restatement(bbme, mf, cells, scale, maxmotion, what, **kw):
    """Device against the numpy restatement (and the restatement against the host mirror): image and range, bit for bit."""
    img, r = _device(mf, cells, scale, maxmotion, **kw)
    exp, exp_range = np_color_cells(cells, mf.orig_width, mf.orig_height, mf.padding_x, mf.padding_y, scale, maxmotion)
    host, host_range = _host(bbme, mf, cells, scale, maxmotion)
    assert host_range == exp_range and np.array_equal(host, exp), (what, scale, maxmotion, "host mirror against numpy")
    assert r is None or r == exp_range, (what, scale, maxmotion, r, exp_range)
    if img is not None and not np.array_equal(img, exp):
        bad = np.argwhere((img != exp).any(-1))
        y, x = bad[0]
        cell = cells[(mf.padding_y + scale * y) >> 1, (mf.padding_x + scale * x) >> 1]
        raise AssertionError("%s scale %d maxmotion %g: %d pixels differ, first (%d, %d) vector %s: device %s numpy %s"
                             % (what, scale, maxmotion, len(bad), x, y, tuple(cell), img[y, x], exp[y, x]))
    return exp_range


@pytest.mark.parametrize("name", list(WIDE))
def test_one_large_vector_in_every_lane_iteration_and_tile(bbme, name):
    """A grid of vectors in [-20, 20] in which ONE cell -- the one sampled column i* of the last sampled row reads -- holds
    (+300, +200) or (-300, -200): max radius and max u / max v (min u / min v) then come from that cell alone, i.e. from lane
    i* % 256 in iteration (i* % 1024) / 256 of range tile i* / 1024, and the image is normalised by it."""
    (w, h, search, block), plan = WIDE[name]
    mf = _zero_mf(bbme, w, h, search, block, plan)
    ch, cw = mf.cells_shape
    base = np.random.default_rng(w).integers(-20, 21, (ch, cw, 2)).astype(np.int16)
    calls = 0
    for scale in (1, 2, 3):
        ncx, ncy = _sampled(mf, scale)
        assert mf.color_shape(scale)[:2] == ((ncy, ncx) if scale > 1 else (h, w))
        base_range = np_color_cells(base, w, h, mf.padding_x, mf.padding_y, scale)[1]
        if scale == 1:
            assert base_range == (float(np.sqrt(np.float32(800))), -20.0, 20.0, -20.0, 20.0)
        columns = [i for i in PROBE_COLUMNS if i < ncx - 1] + [ncx - 1]
        if name == "2100x8":
            assert ncx == (1050, 1050, 700)[scale - 1] and len(columns) == (9, 9, 5)[scale - 1]
        for i in columns:
            for vec in PROBE_VECTORS:
                cells = base.copy()
                cells[_sampled_cell(mf, scale, i, ncy - 1)] = vec
                what = "%s column %d vector %s" % (name, i, vec)
                kw = {}
                if name == "2098x16":                  # 3 x 2098 bytes a row: 6294 + 5 and 6294 + 2 (a multiple of 4: twin rows)
                    kw = dict(pitch_extra=5, offset=3) if vec[0] > 0 else dict(pitch_extra=2, offset=1)
                fixed = i == columns[-2] and vec[0] > 0
                r = _assert_device_equals_restatement(bbme, mf, cells, scale, FIXED if fixed else -1.0, what, **kw)
                # without that cell the range is another one: the comparison above hangs on this one lane-iteration
                lo = vec[0] < 0
                assert r[0] != base_range[0] and r[1 + (not lo)] != base_range[1 + (not lo)] and r[3 + (not lo)] != base_range[3 + (not lo)], what
                assert r[1 + lo] == base_range[1 + lo] and r[3 + lo] == base_range[3 + lo], what
                if name == "2100x8" and scale == 1:
                    assert r == ((float(np.sqrt(np.float32(130000))), -20.0, 300.0, -20.0, 200.0) if not lo else
                                 (float(np.sqrt(np.float32(130000))), -300.0, 20.0, -200.0, 20.0)), what
                if i == columns[-1]:
                    _assert_device_equals_restatement(bbme, mf, cells, scale, -1.0, what + ", range only", want=("range",))
                    _assert_device_equals_restatement(bbme, mf, cells, scale, -1.0, what + ", image only", want=("out",), **kw)
                calls += 1
    assert calls == {"2100x8": 46, "2098x16": 46, "1030x8": 26}[name]
    mf.close()


def test_vectors_over_the_whole_int16_range(bbme):
    """16 x 1050 cells of random int16 vectors with the bounds at known cells, normalised by their own radius (46341), by 7.5, by
    the smallest normal float (u / maxrad overflows to infinity: radius inf, the angle still finite) and by 3e38 (quotients
    underflow: everything at the wheel's centre): device == host mirror == numpy restatement, image and range."""
    mf = _zero_mf(bbme, 2100, 32, [4], [4], (2100, 32, 0, 0))
    cells = full_range_grid()
    assert cells.shape[:2] == mf.cells_shape
    for scale in (1, 3, 4):
        for maxmotion in (-1.0, FIXED) + EXTREME_MAXMOTIONS:
            _assert_device_equals_restatement(bbme, mf, cells, scale, maxmotion, "full range")
    r = _device(mf, cells, 1, -1.0, want=("range",))[1]
    assert r == (float(np.sqrt(np.float32(2) * np.float32(32768) ** 2)), -32768.0, 32767.0, -32768.0, 32767.0)
    mf.close()


def _rolled_beyond(frame, cut, shift=3):
    """The frame with its columns from `cut` on rolled right by `shift` pixels: the true motion there is (+shift, 0)."""
    out = frame.copy()
    out[:, cut:] = np.roll(frame[:, cut:], shift, axis=1)
    return out


def test_every_pairs_range_from_one_launch_on_wide_rows(bbme):
    """bbme_flow_ranges on rows of two range tiles, the pair as blockIdx.y: pair 0 moves from column 400 on, pair 1 only from
    column 2060 on -- its extreme u lies in the second tile alone --, pair 2 not at all."""
    w, h, search, block = 2100, 8, [12], [4]
    assert bbme.plan_padding(w, h, search, block) == (2100, 8, 0, 0)
    f0 = np.random.default_rng(2100).integers(0, 256, (h, w), dtype=np.uint8)
    f1 = _rolled_beyond(f0, 400)
    f2 = _rolled_beyond(f1, 2060)
    video = [f0, f1, f2, f2.copy()]
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(3)], search, block)
    chain = bbme.MFChain(video, search, block)
    for ctx, what in ((batch, "batch"), (chain, "chain")):
        ctx.estimate_async()
        cells = [ctx.get_pair_cells(p) for p in range(3)]
        u = cells[1][..., 0]                               # scale 1, no padding: sampled column i is cell column i
        assert u.max() == 3 and (u[:, :1024] < 3).all() and (u[:, 1024:] == 3).any(), what
        assert cells[0][..., 0].max() == 3 and (cells[0][:, :1024, 0] == 3).any() and not cells[2].any(), what
        for scale in (1, 2, 3):
            exp = [np_color_cells(c, w, h, 0, 0, scale) for c in cells]
            ranges = ctx.flow_ranges_all("forward", scale)
            assert ranges.shape == (3, 5) and ranges.dtype == np.float32
            assert [tuple(float(v) for v in row) for row in ranges] == [e[1] for e in exp], (what, scale)
            for p in range(3):
                assert np.array_equal(ctx.get_pair_flow_color(p, scale), exp[p][0]), (what, scale, p)
                assert ctx.last_color_range == exp[p][1], (what, scale, p)
        assert [tuple(float(v) for v in row)[2] for row in ctx.flow_ranges_all("forward", 1)] == [3.0, 3.0, 0.0], what
        ctx.close()


def test_the_image_buffer_grows_from_call_to_call(bbme):
    """bbme_get_flow_color_host's device image is as large as the largest image asked for so far: smallest first."""
    f1, f2 = _pair(bbme)
    mf = bbme.MF(f1, f2, *MOVING)
    mf.estimate_async()
    cells = mf.get_cells()
    sizes = []
    for scale in (4, 3, 1, 4, 2):
        got = mf.flow_color(scale)
        exp, exp_range = _host(bbme, mf, cells, scale, -1.0)
        assert got.shape == exp.shape and np.array_equal(got, exp), scale
        assert mf.last_color_range == exp_range, scale
        sizes.append(got.size)
    assert sizes[0] < sizes[1] < sizes[2] and sizes[3] < sizes[2]
    mf.close()


def _distinct(field, *images):
    """The first pixel of every distinct vector of the field -> the images' colours there, (n, 3) each."""
    flat = field.reshape(-1, 2)
    _, first = np.unique(flat.view(np.uint32), axis=0, return_index=True)
    return [im.reshape(-1, 3)[first] for im in images]


def _check_against_host_and_reference(bbme, mf, scale, which, cells, field, what):
    flow = bbme.Flow()
    for maxmotion in (-1.0, 1.25):
        got = mf.flow_color(scale, maxmotion, which)
        exp, exp_range = _host(bbme, mf, cells, scale, maxmotion)
        assert got.shape == mf.color_shape(scale) and np.array_equal(got, exp), (what, maxmotion)
        assert mf.last_color_range == exp_range, (what, maxmotion)
        ref = flow.MotionToColor(field, maxmotion, verbose=False)
        assert flow.last_range == exp_range, (what, maxmotion)
        assert_within_atan2_cap(*_distinct(field, got, ref), (what, maxmotion, "distinct vectors"))
    assert mf.flow_range(which, scale) == exp_range


@pytest.mark.parametrize("params", [CHEAP, MOVING], ids=["search4", "search16"])
def test_flow_color_after_a_real_estimate(bbme, params):
    f1, f2 = _pair(bbme)
    mf = bbme.MF(f1, f2, *params)
    mf.estimate_async()
    cells = mf.get_cells()
    if params is MOVING:
        assert len(np.unique(cells.reshape(-1, 2), axis=0)) > 8          # the field carries motion
    for scale in (1, 3, 4):
        _check_against_host_and_reference(bbme, mf, scale, "forward", cells, mf.get_subsampled_flow(scale), ("forward", scale))
    with pytest.raises(bbme.BbmeError) as e:
        mf.flow_color(1, which="backward")
    assert e.value.status == -7                                         # no backward cells have been kept
    mf.estimate_bidirectional_async()
    assert np.array_equal(mf.get_cells(), cells)
    back = mf.get_backward_cells()
    px, py = mf.padding_x, mf.padding_y
    for scale in (1, 4):
        field = np.repeat(np.repeat(back, 2, 0), 2, 1)[py:py + H:scale, px:px + W:scale].astype(np.float32) / np.float32(scale)
        _check_against_host_and_reference(bbme, mf, scale, "backward", back, field, ("backward", scale))
        _check_against_host_and_reference(bbme, mf, scale, "forward", cells, mf.get_subsampled_flow(scale), ("forward again", scale))
    if params is MOVING:
        assert not np.array_equal(mf.flow_color(1, which="backward"), mf.flow_color(1))
    mf.close()


def test_flow_color_of_the_reference_pipeline(bbme):
    """upsample=4 at scale 4: main_class.cpp:32-75 with nothing but the frames going up and the picture coming down."""
    f1, f2 = _pair(bbme, 50, 42, seed=33, max_motion=1)
    mf = bbme.MF(f1, f2, *MOVING, upsample=4)
    mf.estimate_async()
    assert mf.color_shape() == (42, 50, 3)
    cells = mf.get_cells()
    _check_against_host_and_reference(bbme, mf, 4, "forward", cells, mf.get_subsampled_flow(), "x4")
    assert np.array_equal(mf.flow_color(), mf.flow_color(4))
    mf.close()


def test_batch_and_chain_equal_single_contexts(bbme):
    from blockbasedmotionestimation_amd.sequence import colorize_frames
    video = bbme.synth_video(W, H, 5, 77, max_motion=3)
    singles = []
    for p in range(4):
        mf = bbme.MF(video[p], video[p + 1], *MOVING)
        mf.estimate_bidirectional_async()
        s = dict(auto=mf.flow_color(1), fixed=mf.flow_color(3, 2.5), back=mf.flow_color(4, which="backward"))
        s["back_range"] = mf.last_color_range
        s["range1"], s["range3"] = mf.flow_range("forward", 1), mf.flow_range("forward", 3)
        assert np.array_equal(s["auto"], _host(bbme, mf, mf.get_cells(), 1, -1.0)[0])
        singles.append(s)
        mf.close()
    assert len({s["range1"] for s in singles}) > 1
    batch = bbme.MFBatch([(video[p], video[p + 1]) for p in range(3)], *MOVING)
    chain = bbme.MFChain(video[:4], *MOVING)
    for ctx, what in ((batch, "batch"), (chain, "chain")):
        ctx.estimate_bidirectional_async()
        for scale, key in ((1, "range1"), (3, "range3")):
            r = ctx.flow_ranges_all("forward", scale)
            assert r.shape == (3, 5) and r.dtype == np.float32
            assert [tuple(float(v) for v in row) for row in r] == [s[key] for s in singles[:3]], (what, scale)
        assert [tuple(float(v) for v in row) for row in ctx.flow_ranges_all("backward", 4)] == [s["back_range"] for s in singles[:3]], what
        for p in range(3):
            assert np.array_equal(ctx.get_pair_flow_color(p, 1), singles[p]["auto"]), (what, p)
            assert ctx.last_color_range == singles[p]["range1"], (what, p)
            assert np.array_equal(ctx.get_pair_flow_color(p, 3, 2.5), singles[p]["fixed"]), (what, p)
            assert np.array_equal(ctx.get_pair_flow_color(p, 4, which="backward"), singles[p]["back"]), (what, p)
        assert np.array_equal(ctx.flow_color(1), singles[0]["auto"]), what          # the inherited call addresses pair 0
        with pytest.raises(bbme.BbmeError) as e:
            ctx.get_pair_flow_color(3)
        assert e.value.status == -1
        ctx.close()
    images, ranges = colorize_frames(video, *MOVING, in_flight=4, batch=2)
    assert images.shape == (4, H, W, 3) and images.dtype == np.uint8 and ranges.shape == (4, 5)
    for p in range(4):
        assert np.array_equal(images[p], singles[p]["auto"]), p
        assert tuple(float(v) for v in ranges[p]) == singles[p]["range1"], p
    images, ranges = colorize_frames(video, *MOVING, maxmotion=2.5, scale=3, in_flight=1, batch=1)
    for p in range(4):
        assert np.array_equal(images[p], singles[p]["fixed"]), p
        assert tuple(float(v) for v in ranges[p]) == singles[p]["range3"], p
    assert colorize_frames(video[:1], *MOVING)[1].shape == (0, 5)


def test_color_calls_on_a_foreign_stream_change_no_state_and_refuse_bad_arguments(bbme):
    import torch
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    inv, state_err = _capi.ERR_INVALID, _capi.ERR_STATE
    f1, f2 = _pair(bbme)
    mf = bbme.MF(f1, f2, *MOVING)
    rows, cols, _ = mf.color_shape(1)
    ch, cw = mf.cells_shape
    out = torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
    r5 = torch.zeros(5, dtype=torch.float32, device="cuda")
    host_img = np.zeros((rows, cols, 3), np.uint8)
    host_r = (C.c_float * 5)()
    torch.cuda.synchronize()
    ctx, o_, r_ = mf._ctx, C.c_void_p(out.data_ptr()), C.c_void_p(r5.data_ptr())
    # before level 0 has reached 2x2 blocks
    assert L.bbme_flow_color_device(ctx, 0, 0, 1, -1.0, o_, 3 * cols, r_, None) == state_err
    assert L.bbme_get_flow_color_host(ctx, 0, 0, 1, -1.0, host_img.ctypes.data, host_r) == state_err
    assert L.bbme_flow_ranges(ctx, 0, 1, host_r) == state_err
    mf.stage_search(1)
    assert L.bbme_flow_color_device(ctx, 0, 0, 1, -1.0, o_, 3 * cols, r_, None) == state_err
    # a grid the caller brings needs no estimate
    cells = _crafted(mf, "all", seed=3)
    _assert_device_equals_host(bbme, mf, cells, 1, -1.0, "no estimate yet")
    mf.estimate_async()
    assert L.bbme_flow_color_device(ctx, 0, 1, 1, -1.0, o_, 3 * cols, r_, None) == state_err      # no backward cells kept
    assert L.bbme_flow_ranges(ctx, 1, 1, host_r) == state_err
    mf.estimate_bidirectional_async()

    def state():
        return dict(flow=mf.get_flow(), cells=mf.get_cells(), back=mf.get_backward_cells(), fb=mf.consistency_stats("forward", 1),
                    sub=mf.get_subsampled_flow(3))

    before = state()
    # a foreign stream: enqueued behind the context's stream, correct once that stream is synchronised
    side = torch.cuda.Stream()
    mf.estimate_bidirectional_async()
    mf.flow_color_device(out, 1, range=r5, hip_stream_handle=side.cuda_stream)
    side.synchronize()
    exp, exp_range = _host(bbme, mf, before["cells"], 1, -1.0)
    assert np.array_equal(out.cpu().numpy(), exp) and tuple(float(v) for v in r5.cpu()) == exp_range
    _assert_device_equals_host(bbme, mf, cells, 3, FIXED, "side stream", stream=side, pitch_extra=5, offset=1)
    mf.flow_color_device(out, 1, 0.75, "backward", hip_stream_handle=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), _host(bbme, mf, before["back"], 1, 0.75)[0])
    mf.flow_color(4)
    mf.flow_range("backward", 2)
    # the other getters' scratch buffers and the colour calls' are independent; a repeated estimate gives the same bits
    after = state()
    mf.estimate_async()
    again = mf.get_cells()
    for k in before:
        assert np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], k
    assert np.array_equal(again, before["cells"]) and np.array_equal(mf.get_flow(), before["flow"])
    assert np.array_equal(mf.flow_color(1), exp)
    mf.estimate_bidirectional_async()
    # argument errors
    t = torch.from_numpy(cells).cuda()
    c_ = C.c_void_p(t.data_ptr())

    def dev(pair=0, which=0, scale=1, o=o_, pitch=3 * cols, r=r_):
        return L.bbme_flow_color_device(ctx, pair, which, scale, -1.0, o, pitch, r, None)

    def any_cells(c=c_, scale=1, o=o_, pitch=3 * cols, r=r_):
        return L.bbme_cells_color_device(ctx, c, scale, -1.0, o, pitch, r, None)

    assert dev() == 0 and any_cells() == 0 and dev(which=1) == 0
    assert dev(o=None) == 0 and dev(r=None) == 0 and any_cells(o=None) == 0 and any_cells(r=None) == 0
    assert dev(o=None, pitch=0) == 0                                  # a pitch of nothing is not looked at
    assert dev(o=None, r=None) == inv and any_cells(o=None, r=None) == inv
    assert any_cells(c=None) == inv
    for pair in (-1, 1):
        assert dev(pair=pair) == inv
        assert L.bbme_get_flow_color_host(ctx, pair, 0, 1, -1.0, host_img.ctypes.data, host_r) == inv
    for which in (-1, 2):
        assert dev(which=which) == inv
        assert L.bbme_get_flow_color_host(ctx, 0, which, 1, -1.0, host_img.ctypes.data, host_r) == inv
        assert L.bbme_flow_ranges(ctx, which, 1, host_r) == inv
    for scale in (0, -4):
        assert dev(scale=scale) == inv and any_cells(scale=scale) == inv
        assert L.bbme_get_flow_color_host(ctx, 0, 0, scale, -1.0, host_img.ctypes.data, host_r) == inv
        assert L.bbme_flow_ranges(ctx, 0, scale, host_r) == inv
    assert dev(pitch=3 * cols - 1) == inv and any_cells(pitch=3 * cols - 1) == inv
    assert dev(scale=2, pitch=3 * ((cols + 1) // 2)) == 0 and dev(scale=2, pitch=3 * ((cols + 1) // 2) - 1) == inv
    assert L.bbme_get_flow_color_host(ctx, 0, 0, 1, -1.0, None, None) == inv
    assert L.bbme_get_flow_color_host(ctx, 0, 0, 1, -1.0, None, host_r) == 0 and tuple(host_r) == exp_range
    assert L.bbme_get_flow_color_host(ctx, 0, 0, 1, -1.0, host_img.ctypes.data, None) == 0 and np.array_equal(host_img, exp)
    assert L.bbme_flow_ranges(ctx, 0, 1, None) == inv
    for null_call in (lambda: L.bbme_flow_color_device(None, 0, 0, 1, -1.0, o_, 3 * cols, r_, None),
                      lambda: L.bbme_cells_color_device(None, c_, 1, -1.0, o_, 3 * cols, r_, None),
                      lambda: L.bbme_get_flow_color_host(None, 0, 0, 1, -1.0, host_img.ctypes.data, host_r),
                      lambda: L.bbme_flow_ranges(None, 0, 1, host_r)):
        assert null_call() == inv
    mf.synchronize()
    # the wrappers' tensor checks
    for bad_out in (out[:, :cols - 1], out[:-1], out.to(torch.int8), out.cpu(), torch.zeros((rows, 3, cols), dtype=torch.uint8, device="cuda").permute(0, 2, 1)):
        with pytest.raises(bbme.BbmeError) as e:
            mf.flow_color_device(bad_out, 1)
        assert e.value.status == inv
    for bad_cells in (t[:, :cw - 2], t.to(torch.int32), t.cpu()):
        with pytest.raises(bbme.BbmeError) as e:
            mf.cells_color_device(bad_cells, out=out, scale=1)
        assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.flow_color_device(out, 1, range=torch.zeros(4, dtype=torch.float32, device="cuda"))
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.flow_color(1, out=np.zeros((rows, cols), np.uint8))
    assert e.value.status == inv
    with pytest.raises(bbme.BbmeError) as e:
        mf.flow_color(1, which="sideways")
    assert e.value.status == inv
    final = state()
    for k in before:
        assert np.array_equal(before[k], final[k]) if isinstance(before[k], np.ndarray) else before[k] == final[k], k
    mf.close()


def test_cli_writes_the_backward_colour_image(bbme, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    f1, f2 = _pair(bbme, 52, 44, seed=35, max_motion=1)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    base = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm"), "--levels", "2", "--block", "8", "--search", "16"]
    r = subprocess.run(base + ["--backward-color", str(tmp_path / "back.ppm"), "--color", str(tmp_path / "fwd.ppm")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, *MOVING, upsample=4)
    mf.estimate_bidirectional_async()
    img = mf.flow_color(which="backward")
    assert img.shape == (44, 52, 3)
    assert (tmp_path / "back.ppm").read_bytes() == b"P6\n52 44\n255\n" + img[..., ::-1].tobytes()
    fwd = bbme.Flow().MotionToColor(mf.get_subsampled_flow(), verbose=False)      # --color stays the host's route
    assert (tmp_path / "fwd.ppm").read_bytes() == b"P6\n52 44\n255\n" + fwd[..., ::-1].tobytes()
    mf.close()
    r = subprocess.run(base + ["--no-upsample", "--backward-color", str(tmp_path / "plain.ppm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, *MOVING)
    mf.estimate_bidirectional_async()
    img = mf.flow_color(1, which="backward")
    assert (tmp_path / "plain.ppm").read_bytes() == b"P6\n52 44\n255\n" + img[..., ::-1].tobytes()
    mf.close()
    r = subprocess.run(base + ["--backward-color"], capture_output=True, text=True)
    assert r.returncode == 2 and "--backward-color" in r.stderr
