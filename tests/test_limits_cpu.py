"""The premises of tests/test_gpu_limits.py, proven without a GPU: the content generated in helpers.py really drives block SADs
to the ceiling 255 B^2, really has non-trivial winners, the dented blocks really win with the candidates of the highest spiral
ranks, the injected grids really push energies beyond 2^24 and vectors to the bounds of their packings.  Checked with the CPU
oracle and plain numpy int64 sums.  A GPU case whose premise is not asserted here does not belong in test_gpu_limits.py."""
import numpy as np
import pytest

import helpers as H


def _range(c, lvl=0):
    return (c["search"][lvl] - c["block"][lvl]) // 2


def _block_sad(p1, p2, y0, x0, b, dx, dy):
    a = p1[y0:y0 + b, x0:x0 + b].astype(np.int64)
    c = p2[y0 + dy:y0 + dy + b, x0 + dx:x0 + dx + b].astype(np.int64)
    assert c.shape == (b, b), "candidate outside the plane"
    return int(np.abs(a - c).sum())


def _valid_window(box, y0, x0, R):
    """Box sums of the candidates of the block at (y0, x0) that lie inside the plane (the others are skipped, :335)."""
    return box[max(0, y0 - R):y0 + R + 1, max(0, x0 - R):x0 + R + 1]


@pytest.mark.parametrize("name", [n for n, c in H.LIMIT_CONTENTS.items() if c["family"] != "dent"])
def test_ceiling_families_have_real_winners_at_the_ceiling(oracle, name):
    c = H.LIMIT_CONTENTS[name]
    p1, p2 = H.limit_content_planes(name)
    exp, _, _ = H.oracle_stages_from_planes(oracle, p1, p2, c["search"], c["block"], c["raster"])
    searches = [e for e in exp if e[0] == "search"]
    assert len(searches) == len(c["block"])
    for _, lvl, b, mvs in searches:
        nonzero = (mvs != 0).any(-1).mean()
        assert nonzero >= 0.5, "%s level %d: only %.0f %% of the blocks win with a non-zero vector" % (name, lvl, 100 * nonzero)
    # the coarsest level searches around a zero prediction: its sums can be restated in numpy
    lvl = len(c["block"]) - 1
    _, _, b, mvs = searches[0]
    a, img2 = p1[lvl], p2[lvl]
    R, ceiling = _range(c, lvl), 255 * b * b
    h, w = a.shape
    if c["family"] == "inverse_binary":
        for r in range(mvs.shape[0]):
            for q in range(mvs.shape[1]):
                assert _block_sad(a, img2, r * b, q * b, b, 0, 0) == ceiling           # the zero vector: exactly the ceiling
                dx, dy = mvs[r, q]
                assert _block_sad(a, img2, r * b, q * b, b, dx, dy) < 0.6 * ceiling     # the winner: about half of it
        return
    # image1 constant: SAD = |255 b^2 [image1 = 255] - box sum of image2|, int64
    box = H.box_sums(img2, b)
    sad = box if c["family"] == "dark_on_bright" else ceiling - box
    largest, distinct = 0, 0
    for r in range(mvs.shape[0]):
        for q in range(mvs.shape[1]):
            win = _valid_window(sad, r * b, q * b, R)
            largest = max(largest, int(win.max()))
            dx, dy = mvs[r, q]
            assert abs(dx) <= R and abs(dy) <= R
            assert sad[r * b + dy, q * b + dx] == win.min(), "the oracle's winner is not an arg-min of the int64 sums"
            distinct += int(win.min() < win.max())
    assert ceiling - 3 * b * b <= largest <= ceiling, (largest, ceiling)
    assert int(sad.min()) >= ceiling - 3 * b * b                                       # EVERY sum is within 3 b^2 of the ceiling
    assert distinct == mvs.shape[0] * mvs.shape[1]                                     # no block in which all candidates tie


@pytest.mark.parametrize("name", [n for n, c in H.LIMIT_CONTENTS.items() if c["family"] == "dent"])
def test_dented_blocks_win_with_the_outermost_candidates(oracle, name):
    c = H.LIMIT_CONTENTS[name]
    (p1,), (p2,) = H.limit_content_planes(name)
    b, R = c["block"][0], _range(c)
    ceiling = 255 * b * b
    exp, _, _ = H.oracle_stages_from_planes(oracle, [p1], [p2], c["search"], c["block"])
    mvs = exp[0][3]
    box = H.box_sums(p2, b)                                  # image1 = 0: the SADs themselves
    assert int(box.max()) == ceiling
    dx_s, dy_s = oracle.spiral_walk(c["search"][0] - c["block"][0])
    rank = {(int(x), int(y)): k for k, (x, y) in enumerate(zip(dx_s, dy_s))}
    assert len(rank) == (2 * R + 1) ** 2
    for br, bc, sx, sy in c["dents"]:
        y0, x0 = br * b, bc * b
        assert y0 - R >= 0 and x0 - R >= 0 and y0 + R + b <= p2.shape[0] and x0 + R + b <= p2.shape[1], "not an interior block"
        assert tuple(mvs[br, bc]) == (sx * R, sy * R), (name, br, bc, tuple(mvs[br, bc]))
        win = _valid_window(box, y0, x0, R)
        assert win.shape == (2 * R + 1, 2 * R + 1)
        want = ceiling - (1 if sx and sy else b)
        assert win[R + sy * R, R + sx * R] == want == win.min() and int((win == want).sum()) == 1   # a unique winner ...
        if sx and sy:
            assert int((win == ceiling).sum()) == win.size - 1                          # ... every other candidate at the ceiling
        assert rank[(sx * R, sy * R)] >= (2 * R - 1) ** 2                               # ... on the outermost ring of the spiral
    if name.endswith("r63"):
        assert rank[(63, -63)] == 16128 and any((sx, sy) == (1, -1) for _, _, sx, sy in c["dents"])   # the highest rank there is


def test_every_gpu_search_and_regulariser_case_uses_a_proven_content():
    names = set(H.LIMIT_CONTENTS)
    assert {n for n, _ in H.LIMIT_SEARCH_CASES} <= names and set(H.LIMIT_REG_CONTENTS) <= names
    assert set(H.LIMIT_BATCH_CONTENTS) <= names and set(H.LIMIT_SPEC_CONTENTS) <= names
    geo = {(H.LIMIT_CONTENTS[n]["w"], H.LIMIT_CONTENTS[n]["h"], tuple(H.LIMIT_CONTENTS[n]["search"]),
            tuple(H.LIMIT_CONTENTS[n]["block"])) for n in H.LIMIT_BATCH_CONTENTS}
    assert len(geo) == 1 and len(H.LIMIT_CONTENTS[H.LIMIT_BATCH_CONTENTS[0]]["block"]) == 1    # one context, one level
    for n, c in H.LIMIT_CONTENTS.items():                     # no padding: the injected planes are the whole level
        top = len(c["block"]) - 1
        assert c["w"] % (c["block"][top] << top) == 0 and c["h"] % (c["block"][top] << top) == 0, n


@pytest.mark.parametrize("b", H.ENERGY_BLOCKS)
def test_injected_energies_exceed_2_pow_24(oracle, b):
    g = H.ENERGY_LEVEL
    B = g["block"][0]
    p1, p2, field = H.energy_case(b)
    omf = oracle.OracleMF(search_size=g["search"], block_size=g["block"], planes1=p1, planes2=p2)
    after = [H.oracle_sweeps_from_grid(oracle, omf, 0, B, b, field, mults) for mults in H.ENERGY_RUNS]
    omf.close()
    lam = np.float32(H.level_lambda(B, b))
    ys, xs = np.mgrid[1:field.shape[0] - 1, 1:field.shape[1] - 1] * b
    c = field[1:-1, 1:-1].astype(np.int64)
    inside = (xs + c[..., 0] >= 0) & (xs + c[..., 0] <= g["w"] - b) & (ys + c[..., 1] >= 0) & (ys + c[..., 1] <= g["h"] - b)
    assert inside.mean() > 0.5, "the vectors are mostly inside the plane"
    for mults in H.ENERGY_RUNS:                              # the first sweep of each run starts from the injected grid
        terms = H.smoothness_terms(field, lam * np.float32(mults[0]))
        beyond = (terms > 2.0 ** 24) & inside
        assert beyond.sum() >= 0.05 * inside.sum(), (b, mults, int(beyond.sum()))
    # and the sweeps have work to do: a field that no sweep changes would test nothing
    for run in after:
        assert (run[0] != field).any(-1).mean() > 0.3
    assert (after[0][1] != after[0][0]).any() and (after[1][0] != after[0][0]).any()
    # the SADs stay far below 2^24: what breaks float32 exactness is the smoothness term alone
    assert 255 * b * b < 2 ** 15


@pytest.mark.parametrize("b", H.ENERGY_BLOCKS)
def test_tie_fields_make_float32_rounding_decide(oracle, b):
    """The "ties" grid: lambda * mult is a power of two, so lambda * mult * S is exact in float32 and candidates with different S
    lie whole multiples of it apart -- rounding can only decide between candidates of EQUAL S.  This grid has them: blocks where
    the float32 energies of two candidates tie or swap although their exact sums differ."""
    g = H.ENERGY_LEVEL
    B = g["block"][0]
    p1, p2, field = H.energy_case(b, "ties")
    assert {tuple(v) for v in field.reshape(-1, 2).tolist()} == set(H.TIE_VECTORS)
    for mults in H.ENERGY_RUNS:
        blocks, differ = H.tie_field_float_vs_exact(p1[0], p2[0], b, field, np.float32(H.level_lambda(B, b)) * np.float32(mults[0]))
        assert blocks >= 0.05 * field.shape[0] * field.shape[1] and differ >= 5, (b, mults, blocks, differ)
    omf = oracle.OracleMF(search_size=g["search"], block_size=g["block"], planes1=p1, planes2=p2)
    after = H.oracle_sweeps_from_grid(oracle, omf, 0, B, b, field)
    omf.close()
    assert (after[0] != field).any(-1).mean() > 0.3 and (after[1] != after[0]).any()


@pytest.mark.parametrize("name", list(H.GUARD_CASES))
def test_memo_guard_fields_reach_the_14_bit_bound(oracle, name):
    w, h, memo_allowed = H.GUARD_CASES[name]
    p1, p2, f = H.guard_case(name)
    b = H.GUARD_BLOCK
    ys, xs = np.mgrid[0:f.shape[0], 0:f.shape[1]] * b
    x2, y2 = xs + f[..., 0], ys + f[..., 1]
    assert (x2 >= 0).all() and (x2 <= w - b).all() and (y2 >= 0).all() and (y2 <= h - b).all()   # every candidate's own block inside
    top = int(np.abs(f.astype(np.int64)).max())
    assert top == max(w, h) - b
    assert (top <= 8191) == memo_allowed == (max(w, h) <= 8192)          # 14 signed bits hold +-8191: beyond the guard they do not
    omf = oracle.OracleMF(search_size=[H.GUARD_SEARCH], block_size=[b], planes1=p1, planes2=p2)
    after = H.oracle_sweeps_from_grid(oracle, omf, 0, b, b, f)
    omf.close()
    assert (after[0] != f).any(-1).mean() > 0.3 and (after[1] != after[0]).any()
    if not memo_allowed:
        assert int((np.abs(f.astype(np.int64)) > 8191).any(-1).sum()) >= 8      # candidates that 14 bits cannot hold


@pytest.mark.parametrize("b", [16, 8, 2])
def test_int16_bound_vectors_are_outside_and_the_oracle_takes_them(oracle, b):
    g = H.INT16_LEVELS
    p1, p2, f = H.int16_case(b)
    have = {tuple(v) for v in f.reshape(-1, 2).tolist()}
    assert set(H.INT16_SPECIALS) <= have and (-32768, -32768) in have
    omf = oracle.OracleMF(search_size=g["search"], block_size=g["block"], planes1=p1, planes2=p2)
    after = H.oracle_sweeps_from_grid(oracle, omf, 1, g["block"][1], b, f)
    assert (after[0] != f).any()
    special = np.abs(f.astype(np.int64)).max(-1) >= 16384
    # such a candidate lies outside the plane and scores FLT_MAX (:578-580): it never spreads, but a block whose nine candidates
    # are all outside keeps its own (first strict minimum)
    assert not (np.abs(after[1]).max(-1) >= 16384)[~special].any()
    if b == 2:
        # copyMVs doubles the vector in float (:836): +-65534 and +-32768 are exact there, the block they predict leaves the plane
        # and takes a zero vector without a search (:304-310)
        got = H.oracle_search_from_coarse(omf, f, g["block"][1], g["block"][0])
        B0, B1 = g["block"][0], g["block"][1]
        hit = 0
        for r in range(got.shape[0]):
            for q in range(got.shape[1]):
                cv = f[((r * B0) // (2 * B1)) * B1 // 2, ((q * B0) // (2 * B1)) * B1 // 2]
                if np.abs(cv.astype(np.int64)).max() >= 16384:
                    assert tuple(got[r, q]) == (0, 0)
                    hit += 1
        assert hit >= 4 and (got != 0).any()
    omf.close()


def test_ceiling_content_estimates_a_zero_field(oracle):
    """The motion-compensation statistics at saturation need a zero field on image1 = 0 / image2 = 255 (and the mirror): all
    candidates tie there and the first one, the zero vector, wins every search and every sweep."""
    for flip in (False, True):
        (p1,), (p2,) = H.limit_planes("ceiling", 256, 192, 1, 0)
        if flip:
            p1, p2 = p2, p1
        omf = oracle.OracleMF(p1, p2, [20], [16])
        assert not omf.calc_motion_block_matching().any()
        omf.close()
    assert 3840 * 2160 * 255 * 255 > 2 ** 32 > 64 * 4 * 4 * 255 * 255        # the totals need 64 bits, a wave's share does not


@pytest.mark.parametrize("kind", ["plain", "holes", "unknown"])
@pytest.mark.parametrize("scale", [1, 3])
def test_epe_reference_is_the_oracles_calculate_mse(oracle, kind, scale):
    """helpers.epe_reference (numpy, float32 per pixel, float64 sum) against the oracle's C restatement of Flow::CalculateMSE on
    the subsampled field -- the project's tolerance for another order of the float64 sum, or both NaN."""
    rng = np.random.default_rng(5 + scale)
    ph, pw, pad_x, pad_y = 96, 128, 4, 2
    cells = rng.integers(-40, 41, (ph // 2, pw // 2, 2)).astype(np.int16)
    gh, gw = -(-(ph - 2 * pad_y) // scale), -(-(pw - 2 * pad_x) // scale)
    gt = H.epe_ground_truth(gh, gw, kind, rng)
    dense = np.repeat(np.repeat(cells, 2, 0), 2, 1).astype(np.float32)
    sub = (dense[pad_y:ph - pad_y:scale, pad_x:pw - pad_x:scale] / np.float32(scale)).astype(np.float32)
    assert sub.shape == gt.shape
    want, got = oracle.calculate_mse(gt, sub), H.epe_reference(gt, cells, pad_x, pad_y, scale)
    if kind == "unknown":
        assert np.isnan(want) and np.isnan(got)
    else:
        assert got == pytest.approx(want, rel=1e-12) and np.isfinite(got)
        if kind == "holes":
            assert got > 1e5                                   # the known values next to 1e9 were counted, not skipped
            assert np.isinf(gt).any() and np.isnan(gt).any() and (np.abs(gt[np.isfinite(gt)]) > 1e9).any()
