"""Shared helpers of the parity tests: drive the product (HIP, through the C-ABI) and the
oracle (CPU restatement) through the reference's level schedule stage by stage."""
import numpy as np
import pytest


# ---- small helpers the GPU test modules share -------------------------------------------------------------------------------
def _stats_of(keys):
    """-> _stats(d): a statistics dict's values in the order of `keys` (every product's test module binds its own STAT_KEYS)."""
    def _stats(d):
        return tuple(d[k] for k in keys)
    return _stats


def _odd_window(mf):
    cx0, cy0, cw, ch = mf.default_cell_window()
    return (cx0 + 3, cy0 + 1, cw - 8, ch - 5)


def _status(bbme, call):
    with pytest.raises(bbme.BbmeError) as e:
        call()
    return e.value.status


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _embed(plane, H0, W0, fill=0):
    out = np.full((H0, W0), fill, plane.dtype)
    out[:plane.shape[0], :plane.shape[1]] = plane
    return out


def _write_pgm(path, img):
    h, w = img.shape
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h) + img.tobytes())


def oracle_schedule(omf, levels, on_stage=None):
    """MF::calcMotionBlockMatching's loop (motion_framework.cpp:115-206) on the oracle,
    reporting every intermediate MV grid: on_stage(name, level, block, mvs int32 (rows, cols, 2))."""
    L = levels
    for lvl in range(L - 1, -1, -1):
        B = omf.block_size(lvl)
        if lvl != L - 1:
            omf.copy_mvs(lvl)
        omf.calc_level_bm(lvl)
        if on_stage:
            on_stage("search", lvl, B, omf.block_mvs(lvl, B))
        b, lam = B, float(B // 2)
        while b > 1:
            for mult in (1, 2):
                omf.set_block_size(lvl, b)
                omf.set_lambda(lvl, lam)
                omf.regularize_mvs(lvl, mult)
                if on_stage:
                    on_stage("sweep%d" % mult, lvl, b, omf.block_mvs(lvl, b))
            omf.divide_blocks(lvl)
            b >>= 1
            lam *= 2
        omf.set_block_size(lvl, B)
    omf.set_block_size(0, 2)
    omf.copy_to_all_pixels(0)
    return omf.flow(0).copy()


def gpu_schedule(mf, levels, blocks, on_stage=None):
    """The same schedule on the product, one C-ABI stage call at a time."""
    for lvl in range(levels - 1, -1, -1):
        B = blocks[lvl]
        mf.stage_search(lvl)
        if on_stage:
            on_stage("search", lvl, B, mf.stage_get_mvs(lvl, B).astype(np.int32))
        b = B
        while b > 1:
            for mult in (1, 2):
                mf.stage_regularize(lvl, b, mult)
                if on_stage:
                    on_stage("sweep%d" % mult, lvl, b, mf.stage_get_mvs(lvl, b).astype(np.int32))
            b >>= 1
    mf.stage_expand()
    return mf.get_flow()


def compare_stagewise(bbme, oracle, f1, f2, search, block, use_planes=True, raster=False):
    """Runs both sides stage by stage on the same planes; asserts every grid is identical.
    Returns (flow_gpu, flow_oracle)."""
    L = len(block)
    omf = oracle.OracleMF(f1, f2, search, block)
    mf = bbme.MF(f1, f2, search, block, L)
    if raster:
        omf.set_raster_search(True)
        mf.set_search_mode(True)
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == \
           (omf.padded_width, omf.padded_height, omf.padding_x, omf.padding_y)
    if use_planes:
        # hand the oracle's planes to the kernels so that pyramid construction (host prep; pyrDown is
        # OpenCV's and not pinned) cannot leak into hot-path parity
        for lvl in range(L):
            mf.set_level_planes(lvl, omf.image(lvl, 1), omf.image(lvl, 2))
    exp = []
    oflow = oracle_schedule(omf, L, lambda *a: exp.append(a))
    got = []
    gflow = gpu_schedule(mf, L, block, lambda *a: got.append(a))
    assert len(exp) == len(got)
    for (en, el, eb, ev), (gn, gl, gb, gv) in zip(exp, got):
        assert (en, el, eb) == (gn, gl, gb)
        bad = np.argwhere((ev != gv).any(-1))
        assert bad.size == 0, "stage %s level %d block %d: %d of %d MVs differ, first at %s: oracle %s gpu %s" % (
            en, el, eb, len(bad), ev.shape[0] * ev.shape[1], bad[0], ev[tuple(bad[0])], gv[tuple(bad[0])])
    assert np.array_equal(oflow, gflow)
    mf.close()
    omf.close()
    return gflow, oflow


# ---- content at the limits of the kernels' packed sums and keys (tests/test_limits_cpu.py proves what it does, ----
# ---- tests/test_gpu_limits.py runs the kernels on it) ------------------------------------------------------------
def limit_pair(family, h, w, rng):
    """One (image1, image2) pair of h x w whose block SADs sit at the ceiling 255 * B * B of any block size B.
    dark_on_bright: image1 = 0, image2 = 255 - U{0..3}: every SAD lies within 3 B^2 of the ceiling, neighbouring candidates
    differ by little and the arg-min is a real one (the variation has to be in image2: with a constant image2 all candidates tie).
    bright_on_dark: its mirror.  inverse_binary: image1 in {0, 255}, image2 = 255 - image1: the zero vector sums to exactly the
    ceiling, everything else to about half of it.  ceiling: image1 = 0, image2 = 255 (the base of dent_planes)."""
    if family == "dark_on_bright":
        return np.zeros((h, w), np.uint8), (255 - rng.integers(0, 4, (h, w))).astype(np.uint8)
    if family == "bright_on_dark":
        return np.full((h, w), 255, np.uint8), rng.integers(0, 4, (h, w)).astype(np.uint8)
    if family == "inverse_binary":
        a = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        return a, (255 - a).astype(np.uint8)
    if family == "ceiling":
        return np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    raise ValueError(family)


def limit_planes(family, w, h, levels, seed):
    """Per-level planes (planes1, planes2), level l being (h >> l) x (w >> l) and generated on its own: a pyrDown of such
    planes would wash the structure out, so coarse levels are injected as extreme as level 0."""
    rng = np.random.default_rng(seed)
    pairs = [limit_pair(family, h >> l, w >> l, rng) for l in range(levels)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def dent_planes(w, h, block, rng_r, dents):
    """image1 = 0, image2 = 255 except pixels of 254 ("dents"), one level.  dents = [(block_row, block_col, sx, sy)] with
    sx, sy in {-1, 0, 1}: for sx, sy != 0 ONE pixel at the far corner of that block's search area, which of the block's
    candidates only (sx R, sy R) contains; for (1, 0) / (0, 1) a line of B pixels along the far edge of the search area, which
    only candidate (R, 0) / (0, R) contains whole.  Every other candidate of the block sums to exactly (or, on the lines,
    nearer to) 255 B^2, so the dented block's winner is a candidate of the highest spiral ranks."""
    (p1,), (p2,) = limit_planes("ceiling", w, h, 1, 0)
    B, R = block, rng_r
    for br, bc, sx, sy in dents:
        x0, y0 = bc * B, br * B
        xs = [x0 + R + B - 1] if sx > 0 else [x0 - R] if sx < 0 else list(range(x0, x0 + B))
        ys = [y0 + R + B - 1] if sy > 0 else [y0 - R] if sy < 0 else list(range(y0, y0 + B))
        for y in ys:
            for x in xs:
                assert 0 <= x < w and 0 <= y < h, "dent outside the plane"
                p2[y, x] = 254
    return [p1], [p2]


def oracle_stages_from_planes(oracle, planes1, planes2, search, block, raster=False):
    """The oracle's schedule on injected per-level planes: ([(stage, level, block, mvs)], dense flow, final 2x2 grid per level)."""
    L = len(block)
    omf = oracle.OracleMF(search_size=search, block_size=block, planes1=planes1, planes2=planes2)
    if raster:
        omf.set_raster_search(True)
    exp = []
    flow = oracle_schedule(omf, L, lambda *a: exp.append(a))
    finals = [omf.block_mvs(lvl, 2).copy() for lvl in range(L)]
    omf.close()
    return exp, flow, finals


def make_mf_from_planes(bbme, planes1, planes2, search, block, raster=False):
    """A product context on the same injected planes (create it under the environment knobs of the form to be tested)."""
    L = len(block)
    mf = bbme.MF(planes1[0], planes2[0], search, block, L)
    assert (mf.padded_height, mf.padded_width) == planes1[0].shape, "the limit geometries need no padding"
    if raster:
        mf.set_search_mode(True)
    for lvl in range(L):
        mf.set_level_planes(lvl, planes1[lvl], planes2[lvl])
    return mf


def assert_stages_equal(exp, got, what=""):
    assert len(exp) == len(got)
    for (en, el, eb, ev), (gn, gl, gb, gv) in zip(exp, got):
        assert (en, el, eb) == (gn, gl, gb)
        bad = np.argwhere((ev != gv).any(-1))
        assert bad.size == 0, "%s: stage %s level %d block %d: %d of %d MVs differ, first at %s: oracle %s gpu %s" % (
            what, en, el, eb, len(bad), ev.shape[0] * ev.shape[1], bad[0], ev[tuple(bad[0])], gv[tuple(bad[0])])


def gpu_stages_match(bbme, planes1, planes2, search, block, expected, raster=False, what="", probe=None):
    """The product's schedule on the injected planes, stage by stage against oracle_stages_from_planes' result.
    probe(mf, stage, level, block) runs after every stage (e.g. to read bbme_sweep_stats)."""
    exp, oflow, _ = expected
    mf = make_mf_from_planes(bbme, planes1, planes2, search, block, raster)
    got = []

    def on_stage(*a):
        got.append(a)
        if probe:
            probe(mf, *a[:3])
    gflow = gpu_schedule(mf, len(block), block, on_stage)
    mf.close()
    assert_stages_equal(exp, got, what)
    assert np.array_equal(oflow, gflow), what


def box_sums(img, b):
    """Sum of every b x b window of img, int64 (rows - b + 1, cols - b + 1).  With image1 = 0 the SAD of the candidate whose
    window starts at (y, x) is box_sums(image2, b)[y, x]; with image1 = 255 it is 255 b^2 minus that."""
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    s[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return s[b:, b:] - s[:-b, b:] - s[b:, :-b] + s[:-b, :-b]


def _content(family, w, h, search, block, seed=0, raster=False, dents=None):
    return dict(family=family, w=w, h=h, search=list(search), block=list(block), seed=seed, raster=raster, dents=dents)


# Contents of the limit tests, by name: geometry (no padding needed), search / block per level, family.  R = (search - block) / 2.
LIMIT_CONTENTS = {
    # dark-on-bright: every SAD within 3 B^2 of the ceiling; one level so that the search is the only producer of the first grid
    "dark_b16_r16": _content("dark_on_bright", 256, 192, [48], [16], 11),          # tight plan (n = 33), rim rounds
    "dark_b8_r16": _content("dark_on_bright", 192, 128, [40], [8], 12),
    "dark_b32_r32": _content("dark_on_bright", 384, 256, [96], [32], 13),          # WIDE: u16 sums flushed every 8 rows
    "dark_b16_odd": _content("dark_on_bright", 256, 192, [49], [16], 14),          # odd shift
    "dark_b8_odd": _content("dark_on_bright", 192, 128, [41], [8], 15),
    "dark_b32_odd": _content("dark_on_bright", 384, 256, [97], [32], 16),
    "dark_b16_r15": _content("dark_on_bright", 256, 192, [46], [16], 17),          # odd range: no rim rounds
    "dark_b16_r63": _content("dark_on_bright", 384, 256, [142], [16], 18),         # 16 129 candidates, ranks up to 16 128
    "dark_b8_r63": _content("dark_on_bright", 192, 128, [134], [8], 19),
    "dark_b32_r63": _content("dark_on_bright", 384, 256, [158], [32], 20),
    "dark_b2": _content("dark_on_bright", 128, 96, [10], [2], 21),                 # the generic kernel's block sizes ...
    "dark_b4": _content("dark_on_bright", 128, 96, [12], [4], 22),
    "dark_b64": _content("dark_on_bright", 512, 384, [80], [64], 23),
    "dark_b16_r64": _content("dark_on_bright", 256, 192, [16 + 2 * 64], [16], 24),  # ... and its ranges
    "dark_b16_r127": _content("dark_on_bright", 256, 192, [16 + 2 * 127], [16], 25),
    "dark_b16_raster": _content("dark_on_bright", 256, 192, [48], [16], 26, raster=True),
    "bright_b16_r16": _content("bright_on_dark", 256, 192, [48], [16], 31),
    "bright_b8_r16": _content("bright_on_dark", 192, 128, [40], [8], 32),
    "bright_b32_r32": _content("bright_on_dark", 384, 256, [96], [32], 33),
    "inverse_b16_r16": _content("inverse_binary", 256, 192, [48], [16], 41),
    "inverse_b8_r16": _content("inverse_binary", 192, 128, [40], [8], 42),
    "inverse_b32_r32": _content("inverse_binary", 384, 256, [96], [32], 43),
    "inverse_b64": _content("inverse_binary", 512, 384, [80], [64], 44),
    # the ceiling next to the border: windows leave the plane on every level (R = 32 on 512 x 384, 256 x 192, 128 x 96), so
    # valid 0xFFxx sums and the 0xFFFF mark of an out-of-range column meet in one accumulator
    "border_b16_r32": _content("dark_on_bright", 512, 384, [80, 80, 80], [16, 16, 16], 51),
    "border_b8_r32": _content("dark_on_bright", 256, 256, [72, 72], [8, 8], 52),
    "border_b32_r32": _content("bright_on_dark", 512, 512, [96, 96], [32, 32], 53),
    # multi-level cases for the speculative search and its list (fix-up) kernel
    "spec_b16": _content("dark_on_bright", 512, 384, [48, 48, 48], [16, 16, 16], 61),
    "spec_b8": _content("inverse_binary", 256, 256, [40, 40], [8, 8], 62),
    "spec_b32": _content("dark_on_bright", 512, 512, [96, 96], [32, 32], 63),
    # the exact ceiling with dents: chosen interior blocks whose only candidate below 255 B^2 is (+-R, +-R), (+R, 0) or (0, +R)
    "dent_b16_r16": _content("dent", 256, 192, [48], [16],
                             dents=[(5, 7, 1, 1), (5, 3, -1, -1), (2, 10, 1, -1), (2, 3, -1, 1), (8, 5, 1, 0), (8, 11, 0, 1)]),
    "dent_b8_r16": _content("dent", 192, 128, [40], [8],
                            dents=[(2, 2, 1, 1), (2, 20, -1, -1), (12, 3, 1, -1), (9, 12, -1, 1), (12, 20, 1, 0), (8, 17, 0, 1)]),
    "dent_b32_r32": _content("dent", 512, 384, [96], [32],
                             dents=[(5, 7, 1, 1), (5, 3, -1, -1), (2, 10, 1, -1), (2, 3, -1, 1), (8, 5, 1, 0), (8, 11, 0, 1)]),
    # ... at the highest spiral rank there is, 16 128 = (+63, -63), and the first of the last ring's last side, (-63, -63)
    "dent_b16_r63": _content("dent", 384, 256, [142], [16], dents=[(10, 5, 1, -1), (10, 17, -1, -1)]),
    "dent_b32_r63": _content("dent", 512, 384, [158], [32], dents=[(8, 3, 1, -1), (8, 12, -1, -1)]),
}


def limit_content_planes(name):
    c = LIMIT_CONTENTS[name]
    if c["family"] == "dent":
        return dent_planes(c["w"], c["h"], c["block"][0], (c["search"][0] - c["block"][0]) // 2, c["dents"])
    return limit_planes(c["family"], c["w"], c["h"], len(c["block"]), c["seed"])


_SPLIT_OFF = {"BBME_SEARCH_SPLIT_BLOCKS": "0"}                 # k_search_fast<B, 1>
_SPLIT_ON = {"BBME_SEARCH_SPLIT_BLOCKS": "100000000"}          # k_search_fast<B, 2>: two waves per macroblock
# (content, environment of the context) of the search tests: every stage against the oracle
LIMIT_SEARCH_CASES = (
    [(n, _SPLIT_OFF) for n in LIMIT_CONTENTS if not n.startswith("spec_")] +
    [(n, _SPLIT_ON) for n in ("dark_b16_r16", "dark_b8_r16", "dark_b32_r32", "dark_b16_r63", "dark_b8_r63", "dark_b32_r63",
                              "inverse_b16_r16", "inverse_b32_r32", "bright_b8_r16", "border_b16_r32", "border_b32_r32",
                              "dent_b16_r16", "dent_b8_r16", "dent_b32_r32", "dent_b16_r63", "dent_b32_r63")] +
    [(n, dict(_SPLIT_OFF, BBME_LOOSE_PLAN="1")) for n in ("dark_b16_r16", "dark_b8_r16", "dent_b16_r16", "dent_b8_r16",
                                                            "inverse_b16_r16", "border_b16_r32")] +
    [(n, {"BBME_GENERIC_SEARCH": "1"}) for n in ("dark_b16_r16", "dent_b16_r16", "dent_b32_r63", "inverse_b32_r32")])

# the regulariser's forms, each over all block sizes from B down to 2 (environment of the context; "memo": the SAD memo must
# have been looked up during the sweeps)
LIMIT_REG_CONTENTS = ("dark_b16_r16", "dark_b32_r32", "inverse_b16_r16", "bright_b8_r16", "dark_b64", "border_b16_r32")
LIMIT_REG_FORMS = {
    "pass1_strip": {"BBME_PASS1_STRIP": "1", "BBME_PASS1_LANES_MAX": "0"},
    "pass1_lanes_low": {"BBME_PASS1_LANES_MAX": "0"},
    "pass1_lanes_high": {"BBME_PASS1_LANES_MAX": "100000000"},
    "solve_waves_1": {"BBME_SOLVE_WAVES": "1"},
    "solve_one_wave": {"BBME_SOLVE_WGS": "1", "BBME_SOLVE_WAVES": "1"},       # (a single wave walks every chain)
    "relax_rule": {"BBME_RELAX_RULE": "1,64,2,1"},
    "memo_off": {"BBME_MEMO": "0"},
    "memo_b8": {"BBME_MEMO": "1", "BBME_MEMO_MIN_B": "8", "BBME_MEMO_FORWARD": "0"},
    "memo_b8_forward": {"BBME_MEMO": "1", "BBME_MEMO_MIN_B": "8", "BBME_MEMO_FORWARD": "1"},
}


# the knobs README's table calls result-neutral (test_gpu_context_state.test_result_neutral_knobs; test_launch_plan_cpu checks that
# every geometry's launch plan has the form the knob is about): name, environment of the context, then per geometry
# (w, h, search, block, content kind); each geometry chosen so that the knob's path runs
KNOB_CASES = [
    # the two-wave fix-up list: speculation on, levels of <= 10 000 blocks where the 128-lane plan pays (+-32 at B <= 16)
    ("list_split", {"BBME_LIST_SPLIT": "0", "BBME_SPEC_MIN_GABS": "0"}, [(512, 384, [80, 80, 80], [16, 16, 16], 1),
                                                                       (384, 256, [72, 72], [8, 8], 0),
                                                                       (512, 384, [96, 96], [32, 32], 3)]),
    # pass 1 evaluates itself instead of flagging for the relaxation launch that BBME_RELAX_STEPS forces into every sweep
    # (pass 1 is lazy in the strip form only, which a single pair takes where the grid is too large for the chain form: the 2 x 2
    # grid of 1024 x 576, 147 456 blocks in 512 columns.  The two smaller geometries never reach it: test_launch_plan_cpu.KNOWN_MISSES)
    ("pass1_eager", {"BBME_PASS1_LAZY": "0", "BBME_RELAX_STEPS": "1"}, [(352, 256, [48, 40, 40], [16, 16, 8], 4),
                                                                       (256, 192, [12, 12], [4, 4], 2),
                                                                       (1024, 576, [24, 24], [8, 8], 0)]),
    # natural block order in the strip kernel, on levels whose block counts are not multiples of 8 (the XCD-aware order pads
    # the grid to one): 22 x 14 and 11 x 7, 46 x 26 and 23 x 13 blocks
    ("xcd_natural", {"BBME_XCD_REMAP": "0"}, [(352, 224, [48, 40], [16, 16], 1),
                                              (360, 200, [30, 30], [8, 8], 0)]),
    # the loose plan differs from the tight one for even ranges at B <= 16 (R = 32 here); R = 7, 45, 63 check it elsewhere;
    # shifted noise moves by an odd amount
    ("loose_plan_r32", {"BBME_LOOSE_PLAN": "1"}, [(384, 256, [80, 72], [16, 8], 1), (384, 256, [80, 72], [16, 8], 0)]),
    ("loose_plan_r7_r45_r63", {"BBME_LOOSE_PLAN": "1"}, [(384, 256, [30, 106], [16, 16], 1), (512, 384, [158, 72], [32, 8], 1)]),
    # relaxation launches on every grid, two steps in front of both sweeps
    ("relax_rule", {"BBME_RELAX_RULE": "0,64,2,2"}, [(352, 256, [48, 40, 40], [16, 16, 8], 0),
                                                     (256, 192, [40, 40], [8, 8], 4)]),
    ("local_rounds_1", {"BBME_LOCAL_ROUNDS": "1", "BBME_RELAX_STEPS": "1"}, [(352, 256, [48, 40, 40], [16, 16, 8], 4),
                                                                             (256, 192, [40, 40], [8, 8], 1)]),
    ("local_rounds_32", {"BBME_LOCAL_ROUNDS": "32", "BBME_RELAX_STEPS": "1"}, [(352, 256, [48, 40, 40], [16, 16, 8], 4),
                                                                               (256, 192, [40, 40], [8, 8], 1)]),
    ("no_graph", {"BBME_NO_GRAPH": "1"}, [(352, 256, [48, 40, 40], [16, 16, 8], 0), (320, 240, [24, 24, 160], [4, 8, 16], 3)]),
]

# ---- grids injected with stage_set_mvs: energies beyond 2^24, the SAD memo's 8192 guard, vectors at int16's bounds ----
def inside_field(rows, cols, b, w, h, rng):
    """A (rows, cols, 2) int16 grid of uniformly random vectors that keep every block's own candidate inside the w x h plane."""
    ys, xs = np.mgrid[0:rows, 0:cols] * b
    u = rng.integers(-xs, w - b - xs + 1)
    v = rng.integers(-ys, h - b - ys + 1)
    return np.stack([u, v], -1).astype(np.int16)


def energy_field(rows, cols, b, w, h, rng, huge=0.35):
    """Large vectors, mostly inside the plane; a fraction `huge` of the blocks carries vectors of up to +-12 000 instead (they
    point outside and score FLT_MAX, but they enter every neighbour's smoothness): lambda * mult * S then exceeds 2^24 while
    the SADs stay in the thousands."""
    f = inside_field(rows, cols, b, w, h, rng)
    big = rng.random((rows, cols)) < huge
    f[big] = rng.integers(-12000, 12001, (int(big.sum()), 2))
    return f


def smoothness_terms(field, lam_mult):
    """float32 lambda * mult * S of every interior block's OWN candidate against its eight neighbours (calculate_smoothness,
    motion_framework.cpp:623-644, restated in numpy int64) and whether that candidate lies inside a w x h plane is left to the
    caller: returns the (rows - 2, cols - 2) float32 terms."""
    f = field.astype(np.int64)
    c = f[1:-1, 1:-1]
    s = np.zeros(c.shape[:2], np.int64)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                s += np.abs(f[dy:dy + c.shape[0], dx:dx + c.shape[1]] - c).sum(-1)
    return np.float32(lam_mult) * s.astype(np.float32)


def level_lambda(B, b):
    """lambda of the sweeps at b under a level of B x B blocks: B / 2 at b = B, doubled at every halving (:134-151)."""
    return float(B // 2) * (B // b)


def oracle_sweeps_from_grid(oracle, omf, level, B, b, field, mults=(1, 2)):
    """Sweeps at block size b on the oracle, from an injected grid, one per lambda multiplier in mults: the grid after each (int32)."""
    omf.flow(level)[...] = 0
    omf.flow(level)[::b, ::b, :] = field
    omf.set_block_size(level, b)
    omf.set_lambda(level, level_lambda(B, b))
    out = []
    for mult in mults:
        omf.regularize_mvs(level, mult)
        out.append(omf.block_mvs(level, b).copy())
    omf.set_block_size(level, B)
    return out


ENERGY_LEVEL = dict(w=1024, h=1024, search=[72], block=[64], seed=71)     # one 1024 x 1024 level of 64 x 64 blocks
ENERGY_BLOCKS = (2, 4, 8)
ENERGY_RUNS = ((1, 2), (2,))       # both sweeps in the schedule's order, and the doubled lambda straight on the injected grid


ENERGY_FIELDS = ("random", "ties")
# "ties": every block carries A, B (both inside, at the same L1 distance from C) or C (far outside).  A block whose neighbourhood
# holds as many A as B has S_A = S_B, so the energies of A and B differ by their SADs alone -- less than one ulp of the float32
# sum once lambda * mult * S is beyond 2^24: float32 rounds them to a tie (the first candidate wins) or even flips them, where
# exact arithmetic would take the smaller SAD.
TIE_VECTORS = ((5, -3), (-4, 6), (12000, 12000))


def energy_case(b, kind="random"):
    g = ENERGY_LEVEL
    rng = np.random.default_rng(g["seed"] + b)
    p1 = rng.integers(0, 256, (g["h"], g["w"]), dtype=np.uint8)
    p2 = rng.integers(0, 256, (g["h"], g["w"]), dtype=np.uint8)
    rows, cols = g["h"] // b, g["w"] // b
    if kind == "ties":
        field = np.array(TIE_VECTORS, np.int16)[rng.choice(3, (rows, cols), p=[0.35, 0.35, 0.3])]
    else:
        field = energy_field(rows, cols, b, g["w"], g["h"], rng)
    return [p1], [p2], field


# the SAD memo packs a vector into 2 x 14 bits; the host allows it on levels of at most 8192 x 8192 only
GUARD_CASES = {"wide_8192": (8192, 64, True), "wide_8448": (8448, 64, False),
               "tall_8192": (64, 8192, True), "tall_8448": (64, 8448, False)}
GUARD_BLOCK, GUARD_SEARCH = 16, 24


def guard_case(name):
    """(planes1, planes2, grid at b = 16): vectors of up to +-(size - 16) that keep every candidate's own block inside."""
    w, h, _ = GUARD_CASES[name]
    rng = np.random.default_rng(80 + (w * 3 + h) % 97)
    p1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    p2 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = GUARD_BLOCK
    f = inside_field(h // b, w // b, b, w, h, rng)
    if w > h:
        f[:, 0, 0], f[:, -1, 0] = w - b, -(w - b)
    else:
        f[0, :, 1], f[-1, :, 1] = h - b, -(h - b)
    return [p1], [p2], f


INT16_LEVELS = dict(w=256, h=192, search=[32, 32], block=[16, 16], seed=91)
INT16_SPECIALS = [(32767, 5), (-32767, -32767), (16384, -16384), (-16384, 0), (-32768, -32768), (-32768, 32767), (3, -32768),
                  (32767, 32767)]


def int16_case(b):
    """Two levels of noise planes and a level-1 grid at block size b: small vectors, with INT16_SPECIALS sprinkled in."""
    g = INT16_LEVELS
    rng = np.random.default_rng(g["seed"])
    planes = [(rng.integers(0, 256, (g["h"] >> l, g["w"] >> l), dtype=np.uint8),
               rng.integers(0, 256, (g["h"] >> l, g["w"] >> l), dtype=np.uint8)) for l in range(2)]
    rows, cols = (g["h"] >> 1) // b, (g["w"] >> 1) // b
    f = rng.integers(-3, 4, (rows, cols, 2)).astype(np.int16)
    n = max(len(INT16_SPECIALS), rows * cols // 6)
    for k, i in enumerate(rng.choice(rows * cols, n, replace=False)):
        f[i // cols, i % cols] = INT16_SPECIALS[k % len(INT16_SPECIALS)]
    return [p[0] for p in planes], [p[1] for p in planes], f


def oracle_search_from_coarse(omf, field2, B1, B0):
    """copyMVs + calcLevelBM of level 0 on the oracle from a level-1 grid given at 2 x 2 cells: level 0's grid at B0 (int32)."""
    omf.flow(1)[...] = 0
    omf.flow(1)[::2, ::2, :] = field2
    omf.set_block_size(1, B1)
    omf.copy_mvs(0)
    omf.calc_level_bm(0)
    return omf.block_mvs(0, B0).copy()


def epe_reference(gt, cells, pad_x, pad_y, scale):
    """Flow::CalculateMSE (rw_flow.cpp:309-332) on the field the 2 x 2-cell grid holds at every scale-th pixel of the unpadded
    frame, divided by scale: the float32 per-pixel expression sqrtf(du * du + dv * dv), every operation rounded to float32 on
    its own (numpy fuses nothing), summed in float64 in row order; unknown ground truth (|u| or |v| > 1e9, NaN) is skipped; NaN when nothing
    is known."""
    gt = np.asarray(gt, np.float32)
    gh, gw = gt.shape[:2]
    ys = (pad_y + scale * np.arange(gh)) >> 1
    xs = (pad_x + scale * np.arange(gw)) >> 1
    est = cells[np.ix_(ys, xs)].astype(np.float32) / np.float32(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        known = ~((np.abs(gt[..., 0]) > np.float32(1e9)) | (np.abs(gt[..., 1]) > np.float32(1e9)) |
                  np.isnan(gt[..., 0]) | np.isnan(gt[..., 1]))
        du = (gt[..., 0] - est[..., 0]).astype(np.float32)
        dv = (gt[..., 1] - est[..., 1]).astype(np.float32)
        sq = ((du * du).astype(np.float32) + (dv * dv).astype(np.float32)).astype(np.float32)
        e = np.sqrt(sq).astype(np.float32)
    n = int(known.sum())
    # summed one by one in row order, as the reference's loop does (cumsum adds sequentially; sum() would add pairwise and may
    # leave the reference's double in its last bit)
    return float(np.cumsum(e[known].astype(np.float64))[-1]) / n if n else float("nan")


def epe_ground_truth(gh, gw, kind, rng):
    """A float32 (gh, gw, 2) ground-truth field: plain: finite values; holes: with +-inf, NaN and values just below, at and just
    above the 1e9 threshold of "unknown"; unknown: nothing known."""
    gt = (rng.random((gh, gw, 2)) * 40 - 20).astype(np.float32)
    if kind == "unknown":
        gt[..., 0] = np.where(rng.random((gh, gw)) < 0.5, np.float32(np.nan), np.float32(2e9))
        return gt
    if kind == "holes":
        big = np.float32(1e9)
        vals = [np.inf, -np.inf, np.nan, np.nextafter(big, np.float32(0)), big, np.nextafter(big, np.float32(np.inf)),
                -np.nextafter(big, np.float32(0)), -np.nextafter(big, np.float32(np.inf))]
        flat = gt.reshape(-1)
        idx = rng.choice(flat.size, min(flat.size // 2, 8 * max(1, flat.size // 200)), replace=False)
        for k, i in enumerate(idx):
            flat[i] = vals[k % len(vals)]
    return gt


# one batched context of four pairs, one level, the families mixed pair by pair (whole frames: the level-0 planes of a frame
# that needs no padding are the frame itself)
LIMIT_BATCH_CONTENTS = ("dark_b16_r16", "bright_b16_r16", "inverse_b16_r16", "dent_b16_r16")
# bbme_estimate with the speculative search and its list kernel forced onto every level
LIMIT_SPEC_CONTENTS = ("spec_b16", "spec_b8", "spec_b32")


def block_sads_of_vector(p1, p2, b, vec):
    """int64 SAD of every b x b block of p1 against p2 displaced by vec, and whether the displaced block lies inside the plane."""
    dx, dy = vec
    h, w = p1.shape
    moved, valid = np.zeros((h, w), np.int64), np.zeros((h, w), bool)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    moved[ys, xs] = p2[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    valid[ys, xs] = True
    sad = np.abs(p1.astype(np.int64) - moved).reshape(h // b, b, w // b, b).sum((1, 3))
    return sad, valid.reshape(h // b, b, w // b, b).all((1, 3))


def tie_field_float_vs_exact(p1, p2, b, field, lam_mult):
    """On a "ties" grid: the interior blocks whose neighbourhood holds as many A as B (>= 1) and at least one C, whose common term
    lambda * mult * S is beyond 2^24 and whose A and B candidates are inside; and, of them, those where the order of the float32
    energies of A and B is not the order of the exact sums.  Returns (blocks, blocks where float32 and exact disagree)."""
    A, B, C = TIE_VECTORS

    def count(mask):
        m = mask.astype(np.int64)
        r, c = m.shape
        return sum(m[dy:dy + r - 2, dx:dx + c - 2] for dy in range(3) for dx in range(3))
    na, nb, nc = (count((field == v).all(-1)) for v in TIE_VECTORS)
    d_ab = abs(A[0] - B[0]) + abs(A[1] - B[1])
    d_c = abs(C[0] - A[0]) + abs(C[1] - A[1])
    assert d_c == abs(C[0] - B[0]) + abs(C[1] - B[1])
    t = np.float32(lam_mult) * (nb * d_ab + nc * d_c).astype(np.float32)            # S_A = S_B where na == nb
    sad_a, in_a = block_sads_of_vector(p1, p2, b, A)
    sad_b, in_b = block_sads_of_vector(p1, p2, b, B)
    sad_a, sad_b = sad_a[1:-1, 1:-1], sad_b[1:-1, 1:-1]
    ok = (na == nb) & (na >= 1) & (nc >= 1) & (t > 2.0 ** 24) & in_a[1:-1, 1:-1] & in_b[1:-1, 1:-1]
    e_a, e_b = sad_a.astype(np.float32) + t, sad_b.astype(np.float32) + t           # float32 sums, as :607
    differs = np.sign(sad_a - sad_b) != np.sign(e_a.astype(np.float64) - e_b.astype(np.float64))
    return int(ok.sum()), int((ok & differs).sum())


# ---- the case lists of the parity tests (tests/test_gpu_parity.py: kernels against the oracle; ----
# ---- tests/test_reference_core_cpu.py: the oracle against the reference's compiled core) -----------
CASES = [
    # (width, height, search_size[], block_size[], seed, max_motion)
    (320, 208, [30, 30, 30], [16, 16, 16], 1001, 12),          # cfg1-like: B=16, R=7, 3 levels
    (256, 192, [48], [16], 1002, 14),                           # single level, R=16
    (384, 256, [48, 48, 48], [16, 16, 16], 1003, 24),           # cfg2-like, 3 levels
    (512, 384, [80, 80, 80], [16, 16, 16], 1004, 40),           # R=32 (cfg3's search), windows leave the image
    (256, 256, [72, 72], [8, 8], 1005, 20),                     # cfg4-like: B=8, R=32
    (512, 512, [64, 64, 64], [32, 32, 32], 1006, 30),           # the reference's own literals: B=32, search 64
    (320, 256, [24, 40, 30], [8, 16, 8], 1007, 10),             # different block / search per level
    (200, 120, [30, 30], [16, 16], 1008, 6),                    # needs padding in both dimensions
    (256, 128, [17, 21], [16, 16], 1009, 3),                    # odd shift (search-block odd), tiny ranges
    (128, 128, [16], [16], 1010, 0),                            # search_size == block_size: centre only
    (256, 192, [12, 12], [4, 4], 1011, 5),                      # B=4
    (512, 512, [80, 80], [64, 64], 1012, 10),                   # B=64 (generic search, 64-lane regulariser groups)
    (640, 512, [20, 20, 20, 24, 24], [4, 4, 4, 8, 8], 1013, 30),  # five levels, large coarse-to-fine motion
    (256, 128, [8, 12], [16, 16], 1014, 2),                     # search_size < block_size: centre candidate only
    (250, 130, [30], [16], 1015, 5),                            # odd-looking size, padded both ways (256 x 144)
    (1024, 64, [48, 48], [16, 16], 1016, 12),                   # two block rows at the coarse level, very wide
    (64, 1024, [48, 48], [16, 16], 1017, 12),                   # two block columns, very tall
    # wide ranges: the fast kernel's packed (SAD, rank) keys at their limits (B=32: ranks up to 16128 need 14 bits)
    (512, 384, [120], [32], 1018, 40),                          # B=32, R=44
    (512, 384, [122], [32], 1019, 44),                          # B=32, R=45: 8281 candidates > 2^13
    (512, 384, [123], [32], 1020, 44),                          # B=32, odd shift, R=45
    (384, 384, [158], [32], 1021, 60),                          # B=32, R=63 (largest supported)
    (384, 256, [134], [8], 1022, 60),                           # B=8, R=63
    (384, 256, [142], [16], 1023, 60),                          # B=16, R=63
    # ranges beyond the strip kernel's packed keys (R > 63) take the generic kernel, whose window then needs more LDS than a kernel
    # gets by default (r04; the reference takes any search size, motion_framework.cpp:296-422)
    (384, 256, [16 + 2 * 64], [16], 1025, 60),                  # B=16, R=64: the first range past the strip kernel
    (320, 256, [8 + 2 * 100, 8 + 2 * 70], [8, 8], 1026, 70),    # B=8, R=100 over R=70
    (384, 384, [32 + 2 * 127], [32], 1027, 100),                # B=32, R=127 (largest supported): 286-row window, 87 KB of LDS
    # 2 x 2 blocks as a level's own block size (r04; the generic search kernel with the block in one dword): alone, under 4 x 4, and
    # between two levels of larger blocks (copyMVs from a level that is already at 2 x 2 cells when its search ends)
    (128, 96, [10], [2], 1028, 3),
    (160, 128, [12, 20], [2, 4], 1029, 4),
    (192, 128, [14, 10, 24], [4, 2, 8], 1030, 5),
    # the author's second literal set (main_class.cpp:15-17, commented out there) on the 584 x 388 Middlebury geometry:
    # 32 x 32 blocks over 16 x 16 ones (search_prediction's mixed-size path) and an odd shift, 42 - 32 = 10 -> R = 5
    (584, 388, [32, 32, 42], [16, 16, 32], 1024, 10),
]


RASTER_CASES = [
    (320, 208, [30, 30, 30], [16, 16, 16], 2001, 12),           # B=16, R=7, 3 levels
    (384, 256, [48, 48], [16, 16], 2002, 24),                   # R=16
    (256, 256, [72, 72], [8, 8], 2003, 20),                     # B=8, R=32: windows and predictions leave the image
    (512, 512, [64, 64, 64], [32, 32, 32], 2004, 30),           # the reference's literals
    (256, 192, [12, 12], [4, 4], 2005, 5),                      # B=4
    (256, 128, [17, 21], [16, 16], 2006, 3),                    # odd search - block
]


def _random_case(rng):
    """A random legal configuration and frame pair (small enough for the oracle to take milliseconds)."""
    levels = int(rng.integers(1, 4))
    blocks = [int(rng.choice([2, 4, 4, 8, 8, 16, 16, 32])) for _ in range(levels)]
    # sizes that need no padding keep the search for a legal size trivial; padding is tested elsewhere; every level's width a
    # multiple of four (the kernels move rows as dwords: only 2 x 2 blocks can ask for less)
    m = int(np.lcm.reduce([b << i for i, b in enumerate(blocks)] + [4 << (levels - 1)]))
    w = m * int(rng.integers(max(2, -(-2 * (blocks[-1] << (levels - 1)) // m)), 6))
    h = m * int(rng.integers(max(2, -(-2 * (blocks[-1] << (levels - 1)) // m)), 5))
    w, h = min(w, 768), min(h, 512)
    w, h = max(m * 2, w // m * m), max(m * 2, h // m * m)
    search = [b + 2 * int(rng.integers(0, 20)) + int(rng.integers(0, 2)) for b in blocks]
    kind = int(rng.integers(0, 5))
    if kind == 0:                       # smooth texture + piecewise motion (the bench's recipe)
        from blockbasedmotionestimation_amd.synth import synth_pair
        f1, f2, _ = synth_pair(w, h, int(rng.integers(1 << 30)), max_motion=int(rng.integers(0, 12)))
    elif kind == 1:                     # white noise, shifted
        f1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        f2 = np.roll(f1, (int(rng.integers(-9, 10)), int(rng.integers(-9, 10))), axis=(0, 1))
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
    return f1, f2, search, blocks


def content_pairs():
    """The tie / flat / periodic / noise / large-motion contents of tests/test_gpu_parity.py: (name, f1, f2, search, block, raster)."""
    from blockbasedmotionestimation_amd.synth import synth_pair
    out = []
    z = np.zeros((128, 192), np.uint8)
    c = np.full((128, 192), 77, np.uint8)
    t1, t2, _ = synth_pair(192, 128, 5, max_motion=8)
    out += [("zeros", z, z, [48, 48], [16, 16], False), ("flat", c, c, [30, 30], [16, 16], False),
            ("flat_vs_texture", c, t2, [30, 30], [16, 16], False), ("texture_vs_flat", t1, c, [30, 30], [16, 16], False)]
    y, x = np.mgrid[0:192, 0:256]
    stripes = ((x // 4) % 2 * 200).astype(np.uint8)
    checker = (((x // 8) + (y // 8)) % 2 * 255).astype(np.uint8)
    out += [("stripes", stripes, np.roll(stripes, 3, axis=1), [48, 48], [16, 16], False),
            ("checker", checker, np.roll(checker, (5, -2), axis=(0, 1)), [48, 48], [16, 16], False)]
    rng = np.random.default_rng(7)
    f1 = rng.integers(0, 256, (256, 320), dtype=np.uint8)
    out.append(("large_motion", f1, np.roll(f1, (37, -45), axis=(0, 1)), [80, 80, 80], [16, 16, 16], False))
    rng = np.random.default_rng(12)
    n1 = rng.integers(0, 256, (160, 224), dtype=np.uint8)
    n2 = rng.integers(0, 256, (160, 224), dtype=np.uint8)
    out.append(("noise_b8", n1, n2, [40, 40], [8, 8], False))
    rng = np.random.default_rng(13)
    n1 = rng.integers(0, 256, (128, 192), dtype=np.uint8)
    n2 = rng.integers(0, 256, (128, 192), dtype=np.uint8)
    out.append(("noise_b4", n1, n2, [24, 24], [4, 4], False))
    rng = np.random.default_rng(14)
    g1 = (rng.integers(0, 3, (128, 192)) * 100).astype(np.uint8)
    g2 = (rng.integers(0, 3, (128, 192)) * 100).astype(np.uint8)
    out.append(("three_grey_levels", g1, g2, [30, 30], [8, 8], False))
    # raster mode where its rules differ from the spiral's (test_raster_search_ties_and_outside_predictions)
    z90 = np.full((128, 192), 90, np.uint8)
    rng = np.random.default_rng(17)
    r1 = rng.integers(0, 256, (256, 320), dtype=np.uint8)
    out += [("raster_flat", z90, z90, [48, 48], [16, 16], True),
            ("raster_stripes", stripes, np.roll(stripes, 3, axis=1), [48, 48], [16, 16], True),
            ("raster_large_motion", r1, np.roll(r1, (37, -45), axis=(0, 1)), [80, 80, 80], [16, 16, 16], True),
            ("raster_three_grey_levels", g1, g2, [30, 30], [8, 8], True)]
    return out


CONTENT_NAMES = ["zeros", "flat", "flat_vs_texture", "texture_vs_flat", "stripes", "checker", "large_motion", "noise_b8",
                 "noise_b4", "three_grey_levels", "raster_flat", "raster_stripes", "raster_large_motion",
                 "raster_three_grey_levels"]


# ---- the cases of tests/test_gpu_reference.py: the kernels against what the reference's compiled core (oracle/_ref/mf_ref) ----
# ---- wrote.  tests/golden/make_golden.py runs mf_ref on these inputs and records sha256 digests of the inputs, of every -------
# ---- stage's grid (as int16) and of the dense field (float32) in tests/golden/reference_digests.json -------------------------
def sha256_of(*arrays):
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def pyramid_planes(oracle, f1, f2, block):
    """The level planes MF::MF makes of a frame pair (zero padding by the plan :14-54, then pyrDown per level), by the oracle's
    host functions: inputs of the comparisons, covered by the recorded input digest."""
    rc, pw, ph, px, py = oracle.plan_padding(f1.shape[1], f1.shape[0], block)
    assert rc == 0, "no padding plan for %s with %s" % (f1.shape, block)
    p1, p2 = [oracle.pad_zero(f1, px, py)], [oracle.pad_zero(f2, px, py)]
    for _ in block[1:]:
        p1.append(oracle.pyr_down(p1[-1]))
        p2.append(oracle.pyr_down(p2[-1]))
    return p1, p2


# name: (source, key): "case" / "raster" index CASES / RASTER_CASES, "content" a CONTENT_NAMES entry.  Every search kernel and
# regulariser form is touched: the strip kernels for B = 8, 16, 32, the generic kernel for 2 x 2, 4 x 4 and 64 x 64 blocks and
# for R = 64 (its first range), the widest strip range R = 63, mixed block sizes between levels, raster mode, ties, predictions
# that leave the image
REF_STAGE_CASES = {
    "cfg1_like": ("case", 0), "cfg4_like_b8_r32": ("case", 4), "literals_b32_s64": ("case", 5), "mixed": ("case", 6),
    "ref2_literals": ("case", 29), "padded": ("case", 7), "odd_shift": ("case", 8), "block2": ("case", 26),
    "block2_under_4": ("case", 27), "block2_between": ("case", 28), "block4": ("case", 10), "b64": ("case", 11), "b16_r63": ("case", 22), "b16_r64": ("case", 23),
    "raster_b16_r7": ("raster", 0), "raster_b8_r32": ("raster", 2), "raster_odd_shift": ("raster", 5),
    "zeros": ("content", "zeros"), "stripes": ("content", "stripes"), "checker": ("content", "checker"),
    "three_grey_levels": ("content", "three_grey_levels"), "large_motion": ("content", "large_motion"),
    "raster_flat": ("content", "raster_flat"), "raster_large_motion": ("content", "raster_large_motion"),
}
# bbme_estimate whole, the speculative search forced onto every level (BBME_SPEC_MIN_GABS=0): LIMIT_CONTENTS entries
REF_SPEC_CASES = ("spec_b16", "spec_b8")
REF_RANDOM_SEEDS = tuple(range(10))           # of test_random_configurations_twice: default schedule, run twice
REF_SWEEP_FORMS = {"default": {}, "pass1_strip": LIMIT_REG_FORMS["pass1_strip"], "solve_one_wave": LIMIT_REG_FORMS["solve_one_wave"],
                   "memo_b8_forward": LIMIT_REG_FORMS["memo_b8_forward"]}
REF_MC_CASE = "cfg1_like"                     # draw_MVimage / compensation_error after an estimate of this case
REF_MC_FILLS = (0, 255)


def ref_stage_case(oracle, name):
    """(planes1, planes2, search, block, raster) of a REF_STAGE_CASES entry."""
    from blockbasedmotionestimation_amd.synth import synth_pair
    source, key = REF_STAGE_CASES[name]
    if source == "content":
        _, f1, f2, search, block, raster = {p[0]: p for p in content_pairs()}[key]
    else:
        w, h, search, block, seed, mm = (CASES if source == "case" else RASTER_CASES)[key]
        f1, f2, _ = synth_pair(w, h, seed, max_motion=mm)
        raster = source == "raster"
    p1, p2 = pyramid_planes(oracle, f1, f2, block)
    return p1, p2, list(search), list(block), raster


def ref_random_case(oracle, seed):
    """(planes1, planes2, search, block) of random configuration `seed`."""
    f1, f2, search, block = _random_case(np.random.default_rng(9000 + seed))
    p1, p2 = pyramid_planes(oracle, f1, f2, block)
    return p1, p2, search, block


def stage_key(name, level, block):
    return "%s_l%d_b%d" % (name, level, block)


def mc_stats(image1, frame_fill0, frame_fill255):
    """[sse, sad, pixels, skipped] of a draw_MVimage frame against image1; a pixel was skipped where the two fills show."""
    ok = frame_fill0 == frame_fill255
    d = frame_fill0.astype(np.int64) - image1.astype(np.int64)
    return [int((d[ok] ** 2).sum()), int(np.abs(d[ok]).sum()), int(ok.sum()), int((~ok).sum())]


# lambda * (float)mult * S at :607 is (lambda * mult) * S.  With the schedule's own values -- lambda a power of two, mult 1 or 2 --
# every product is exact and no association can show; a block size of 12 (lambda = 6) and multipliers such as 37 or 101 make both
# factors odd multiples, and outliers of a million pixels push S (itself a float32 sum beyond 2^24, so its order of summation
# counts too) to where each product rounds.  A and B are one pixel apart in their distance to the outlier C, so that where a
# neighbourhood holds as many A as B the two energies differ by the SADs and a few units of lambda * mult: within the rounding.
ASSOCIATION_LEVEL = dict(w=1020, h=1020, block=12, seed=101, mults=((37,), (101,), (37, 101), (3,)))
ASSOCIATION_VECTORS = ((5, -3), (-4, 7), (1000000, 1000000))


def association_case():
    """(plane1, plane2, int32 grid at 12 x 12 blocks) of the association check (oracle against reference only: the product takes
    neither this block size nor these multipliers)."""
    g = ASSOCIATION_LEVEL
    rng = np.random.default_rng(g["seed"])
    p1 = rng.integers(0, 256, (g["h"], g["w"]), dtype=np.uint8)
    p2 = rng.integers(0, 256, (g["h"], g["w"]), dtype=np.uint8)
    field = np.array(ASSOCIATION_VECTORS, np.int32)[rng.choice(3, (g["h"] // g["block"], g["w"] // g["block"]), p=[0.35, 0.35, 0.3])]
    return p1, p2, field


# ---- frames for the plane kernels (x4 up-sampling, zero border, pyrDown): content on which a wrong filter weight or a wrong ----
# ---- truncation shows, where a smooth texture would hide it ------------------------------------------------------------------
HARD_CONTENTS = ("noise", "binary", "checker", "ramp_x", "ramp_y", "white")


def hard_content(name, h, w, seed=0):
    """One (h, w) uint8 frame: uniform noise, binary noise of 0 / 255, a checkerboard of period 1 in 0 / 255, a ramp along x or
    along y over the whole value range, constant 255."""
    rng = np.random.default_rng([seed, HARD_CONTENTS.index(name), h, w])
    y, x = np.mgrid[0:h, 0:w]
    if name == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if name == "binary":
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    if name == "checker":
        return (((x + y) & 1) * 255).astype(np.uint8)
    if name == "ramp_x":
        return (x * 255 // max(w - 1, 1)).astype(np.uint8)
    if name == "ramp_y":
        return (y * 255 // max(h - 1, 1)).astype(np.uint8)
    if name == "white":
        return np.full((h, w), 255, np.uint8)
    raise ValueError(name)


# ---- content of the scale tests (tests/test_scale_cpu.py proves what it does, tests/test_gpu_scale.py runs the gather kernels ----
# ---- on it): the smallest planes on which k_mc_reduce's lanes take a second trip through the partials ------------------------
SCALE_G1 = dict(w=2058, h=1038, search=[12], block=[4])      # pads to 2060 x 1040, pad (1, 1): 1030 x 520 cells
SCALE_G2 = dict(w=2058, h=2070, search=[12], block=[4])      # pads to 2060 x 2072: k_fb_consistency's 262 workgroups
SCALE_SEED = 7
SCALE_STRENGTH = 64
SCALE_MC_WINDOW = (37, 21, 1998, 1000)                       # pixels, odd on every side
SCALE_SHIFTS = ((2, -2), (-2, 4), (4, 2), (-4, -2))          # (rows, columns) a video's frame k + 1 is rolled by against frame k


def scale_plane(rng, h, w):
    """Low-amplitude noise: the 2x2 SADs of unrelated cells spread over 0..90, so that a strength of 64 meets every weight and
    three unrelated hypotheses win about a third of the cells each (planes of 0..255 give the filter a weight in 1 cell of 800)."""
    return rng.integers(0, 24, (h, w), dtype=np.uint8)


def scale_frames(h, w, n, seed=SCALE_SEED):
    """n unrelated source frames of low-amplitude noise."""
    rng = np.random.default_rng(seed)
    return [scale_plane(rng, h, w) for _ in range(n)]


def scale_grids(ch, cw, seed=SCALE_SEED):
    """The two cell grids of the injected-grid tests (test_interpolation_cpu.random_grids, reach 5)."""
    from test_interpolation_cpu import random_grids
    return random_grids(ch, cw, np.random.default_rng(seed), reach=5)


def scale_filter_content(h0, w0, seed=SCALE_SEED):
    """(C, P, to_prev, N, to_next) of padded size: three unrelated low-amplitude planes and two random grids; in cell rows 0..7
    both neighbours are C itself under zero vectors (cost 0: weight 8, which noise never gives); in cell rows 8..15 to_next
    points outside (one-sided cells)."""
    from test_interpolation_cpu import random_grids
    rng = np.random.default_rng(seed)
    cur, prev, nxt = (scale_plane(rng, h0, w0) for _ in range(3))
    gp, gn = random_grids(h0 // 2, w0 // 2, rng, reach=5)
    prev[:16], nxt[:16] = cur[:16], cur[:16]
    gp[:8], gn[:8] = 0, 0
    gn[8:16] = (32767, 32767)
    return cur, prev, gp, nxt, gn


def scale_bgr_frames(h, w, seed=SCALE_SEED):
    """Two unrelated B,G,R frames of the source size."""
    rng = np.random.default_rng(seed + 1)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def scale_mc_content(h, w, h0, w0, block, seed=SCALE_SEED):
    """(image1, image2 source frames of 0..255, grid at `block`): vectors of -20..20 drawn per 16 x 16 block and handed down to
    the `block` grid, so that blocks along all four borders leave the plane and the SSE of the rest passes 2^32."""
    from test_motion_compensation_cpu import block_mvs_from_grid
    rng = np.random.default_rng(seed + 2)
    f1 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    f2 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    grid16 = rng.integers(-20, 21, (-(-h0 // 16), -(-w0 // 16), 2)).astype(np.int16)
    return f1, f2, np.ascontiguousarray(block_mvs_from_grid(grid16, 16, block, h0, w0))


def scale_video(h, w, n, seed=SCALE_SEED):
    """n source frames: low-amplitude noise, frame k + 1 = frame k rolled by SCALE_SHIFTS[k] plus fresh noise of 0..7, except in
    a rectangle, another one per frame, of unrelated noise: there the two fields of a pair contradict each other and the filter
    finds few matches, so that no two pairs of a video share a statistic."""
    rng = np.random.default_rng(seed + 3)
    frames = [scale_plane(rng, h, w)]
    for k in range(n - 1):
        f = (np.roll(frames[-1], SCALE_SHIFTS[k % len(SCALE_SHIFTS)], axis=(0, 1)) + rng.integers(0, 8, (h, w))).astype(np.uint8)
        y0, y1, x0, x1 = h * (k + 1) // 9, h * (2 * k + 4) // 9, w * (k + 1) // 7, w * (k + 4) // 7
        f[y0:y1, x0:x1] = scale_plane(rng, y1 - y0, x1 - x0)
        frames.append(f)
    return frames


def scale_groups(w0, h0, runs_per_lane, cells=True):
    """(runs, workgroups, runs in the last workgroup) of a gather kernel whose lanes take runs_per_lane runs of 4 cells (of 4
    pixels with cells=False) along a row: the arithmetic of gather_groups (csrc/bbme_device.hip)."""
    cols, rows = (w0 // 2, h0 // 2) if cells else (w0, h0)
    runs = (cols + 3) // 4 * rows
    per_group = 256 * runs_per_lane
    groups = (runs + per_group - 1) // per_group
    return runs, groups, runs - (groups - 1) * per_group


def stats_differ_pairwise(stats, absent_ok=False, words=(0, 1, 2, 3)):
    """Every one of the four words (or of `words`) differs between any two of the launch's pairs / frames / phases: a partial
    read from the wrong one, or a reduction over the wrong pair's partials, changes every word it touches.  absent_ok: a word
    may be 0 in both (frames that have no previous, or no next, neighbour by construction)."""
    stats = [tuple(s) for s in stats]
    return all(a[k] != b[k] or (absent_ok and a[k] == 0)
               for i, a in enumerate(stats) for b in stats[i + 1:] for k in words)


def scale_cell_windows(pad_x, pad_y, w, h):
    """(default, odd) windows in cells: the cells whose top-left pixel lies in the unpadded frame (MF.default_cell_window), and
    that window cut by another 3, 1, 5 and 4 cells at its left, top, right and bottom."""
    x0, y0 = -(-pad_x // 2), -(-pad_y // 2)
    x1, y1 = -(-(pad_x + w) // 2), -(-(pad_y + h) // 2)
    return (x0, y0, x1 - x0, y1 - y0), (x0 + 3, y0 + 1, x1 - x0 - 8, y1 - y0 - 5)


# ---- global motion and global compensation at scale (tests/test_global_motion_scale_cpu.py proves what the shapes and the content
# ---- do, tests/test_gpu_scale.py runs K16, K17, K18 and K18b on them) ----------------------------------------------------------
GM_WIDE = dict(w=8186, h=130, search=[12], block=[4])        # pads to 8188 x 132, pad (1, 1): 4094 x 66 cells, the rule's widest
GM_TALL = dict(w=130, h=8186, search=[12], block=[4])        # pads to 132 x 8188: 66 x 4094 cells, the rule's tallest
GM_SHAPES = {"G1": SCALE_G1, "WIDE": GM_WIDE, "TALL": GM_TALL}
GM_PADDED = {"G1": (2060, 1040), "WIDE": (8188, 132), "TALL": (132, 8188)}
GM_TOL = 3 << 16


def gm_trips(w0, h0, max_groups):
    """(runs, workgroups, trips, runs of the last trip) of k_vector_histogram: min(ceil(runs / 256), max_groups) workgroups stride
    over the runs of 4 cells, 256 runs per workgroup and trip (vh_groups, csrc/bbme_device.hip)."""
    runs = (w0 // 2 + 3) // 4 * (h0 // 2)
    groups = min((runs + 255) // 256, max_groups)
    trips = (runs + groups * 256 - 1) // (groups * 256)
    return runs, groups, trips, runs - (trips - 1) * groups * 256


def gm_cell_window(cw, ch):
    """A window in cells that starts and ends inside runs of 4"""
    return (1, 1, cw - 3, ch - 2)


def gm_plane_window(w0, h0):
    """A window in pixels, odd on every side"""
    return (3, 1, w0 - 8, h0 - 4)


def gm_scale_grid(ch, cw, seed=SCALE_SEED):
    """The grid of the moments tests -> (grid, model, mask): a zooming and rotating field in quarter pels plus noise of +-2, a
    quarter of the cells overwritten from extreme_grid; the field's true model rounded to Q16; an exclusion mask of 30 %.  Under
    GM_TOL about a third of the cells each is an inlier, an outlier and excluded."""
    from test_global_motion_cpu import affine_cells, extreme_grid, random_mask
    g, true = affine_cells(ch, cw, 4, 3.25, -1.5, 0.001, -0.0007)
    rng = np.random.default_rng(seed + 4)
    g += rng.integers(-2, 3, size=g.shape).astype(np.int16)
    pick = rng.random((ch, cw)) < 0.25
    g[pick] = extreme_grid(ch, cw, seed + 5)[pick]
    model = tuple(int(v) for v in np.rint(true * 65536))
    return g, model, random_mask(ch, cw, seed + 6)


def gm_histogram_grids(ch, cw):
    """(name, grid) of the histogram tests and their exclusion mask"""
    from test_global_motion_cpu import extreme_grid, random_grid, random_mask, uniform_grid
    return (("uniform", uniform_grid(ch, cw)), ("random", random_grid(ch, cw, 1)), ("extreme", extreme_grid(ch, cw, 2))), \
        random_mask(ch, cw, 3)


def gm_scale_planes(h0, w0, seed=SCALE_SEED):
    """Two unrelated padded planes of random bytes"""
    rng = np.random.default_rng(seed + 7)
    return rng.integers(0, 256, (h0, w0), dtype=np.uint8), rng.integers(0, 256, (h0, w0), dtype=np.uint8)


GM_BGR_MODELS = (((20000, 2621, -700, -9000, 700, 2621), (3 << 16, 0, 0, -(2 << 16), 0, 0), (16384 + 3000, 300, 0, -8192, 0, -200)), 1)


def gm_scale_bgr_case(h, w, seed=SCALE_SEED):
    """Three pairs of unrelated colour frames, the three models they are warped under from one launch (and the unit), an odd frame
    window"""
    rng = np.random.default_rng(seed + 8)
    c1 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    c2 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    return c1, c2, GM_BGR_MODELS[0], GM_BGR_MODELS[1], (1, 2, w - 5, h - 3)
