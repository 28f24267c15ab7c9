"""Quarter-pel refinement on the GPU (include/bbme.h, "SUBPEL RULE"): k_subpel_refine gives exactly what bbme_subpel_host gives
(which tests/test_subpel_cpu.py holds to the header's text) on injected planes and grids -- odd paddings, cell rows that end inside
a workgroup's tile, caller pitches, vectors on and past every validity bound, int16 extremes, windows, side streams, 2 Mpixel --
and on the context's own planes and fields in both directions, on batches and chains; the field getter expands and divides as the
driver does; no call changes context state."""
import subprocess

import numpy as np
import pytest

from helpers import _cuda, _stats_of, _write_pgm
from test_subpel_cpu import STAT_KEYS, boundary_grid, cells_to_field, extreme_grid

_stats = _stats_of(STAT_KEYS)

pytestmark = pytest.mark.gpu


def _host(bbme, I1, I2, G, window=None):
    out, st = bbme.subpel_cells(I1, I2, G, window)
    return out, _stats(st)


def _device(mf, I1, I2, G, window=None, pitch_extra=0, stream=None, want=("out", "stats")):
    """cells_subpel_device on host planes and a host grid -> (grid (CH, CW, 2) int16, stats tuple), None where not asked for; the
    output's rows are pitch_extra cells further apart than packed."""
    import torch
    CH, CW = mf.cells_shape
    t1, t2, tg = _cuda(I1), _cuda(I2), _cuda(G)
    out = torch.full((CH, CW + pitch_extra, 2), 0x5555, dtype=torch.int16, device="cuda") if "out" in want else None
    st = torch.zeros(4, dtype=torch.int64, device="cuda") if "stats" in want else None
    torch.cuda.synchronize()
    mf.cells_subpel_device(t1, t2, tg, out=None if out is None else out[:, :CW], stats=st, window=window,
                           stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    mf.synchronize()
    if pitch_extra:                                        # the cells between the rows stay untouched
        assert out is None or bool((out[:, CW:] == 0x5555).all())
    return (None if out is None else out[:, :CW].cpu().numpy(), None if st is None else tuple(st.cpu().tolist()))


def _assert_device_equals_host(bbme, mf, I1, I2, G, window=None, what=None, **kw):
    out, st = _device(mf, I1, I2, G, window, **kw)
    exp = _host(bbme, I1, I2, G, window)
    assert out is None or np.array_equal(out, exp[0]), (what, window, np.argwhere((out != exp[0]).any(-1))[:4])
    assert st is None or st == exp[1], (what, window, st, exp[1])
    return exp


def _random_grid(rng, CH, CW, motion=None, reach=4):
    G = rng.integers(-reach, reach + 1, size=(CH, CW, 2))
    if motion is not None:
        G = G // 2 + motion
    return G.astype(np.int16)


# (w, h, search, block): odd paddings (62 -> 64, 46 -> 48); 132 and 140: 66 and 70 cell columns, neither a multiple of 4 nor of
# the kernel's 32-cell tile, so the last workgroup of every tile row holds 2 or 6 columns; 50 and 49 cell rows: the last tile row
# holds 2 rows or 1
GEOMETRIES = [(62, 46, [24, 24], [8, 8]), (132, 100, [12], [2]), (140, 98, [12], [2]), (200, 120, [20, 20], [8, 8])]


@pytest.mark.parametrize("w,h,search,block", GEOMETRIES)
def test_injected_planes_and_grids(bbme, w, h, search, block):
    import torch
    f1, f2, motion = bbme.synth_pair(w, h, 900 + w, max_motion=4, tiles=3)
    mf = bbme.MF(f1, f2, search, block)
    W0, H0 = mf.padded_width, mf.padded_height
    CH, CW = mf.cells_shape
    if w == 62:
        assert mf.padding_x % 2 == 1 and mf.padding_y % 2 == 1
    if w in (132, 140):
        assert (W0, H0) == (w, h) and CW % 4 != 0 and CW % 32 != 0
    I1, I2 = mf.get_level_planes(0)
    rng = np.random.default_rng(w)
    pm = np.zeros((H0, W0, 2), np.int64)
    pm[mf.padding_y:mf.padding_y + h, mf.padding_x:mf.padding_x + w] = motion
    G = _random_grid(rng, CH, CW, pm[::2, ::2], reach=2)
    win = (CW - 7, 2, 7, CH - 5)                           # reaches the last, cut tile of every tile row
    _, st = _assert_device_equals_host(bbme, mf, I1, I2, G, None, "near the motion")
    assert st[0] > 0.5 * CH * CW and st[1] > 0 and st[3] < st[2]
    _assert_device_equals_host(bbme, mf, I1, I2, G, win, "window, pitch + 1", pitch_extra=1)
    _assert_device_equals_host(bbme, mf, I1, I2, G, (3, 3, 1, 1), "one cell, pitch + 3", pitch_extra=3)
    _assert_device_equals_host(bbme, mf, I1, I2, G, win, "statistics alone", want=("stats",))
    _assert_device_equals_host(bbme, mf, I1, I2, G, None, "grid alone", want=("out",))
    _assert_device_equals_host(bbme, mf, I2, I1, G, None, "side stream", stream=torch.cuda.Stream(), pitch_extra=2)
    _assert_device_equals_host(bbme, mf, I1, I2, _random_grid(rng, CH, CW, reach=12), win, "far vectors")
    B, cells = boundary_grid(W0, H0, 9)
    out, _ = _assert_device_equals_host(bbme, mf, I1, I2, B, None, "validity bounds")
    for cx, cy, ok in cells:
        _, st = _device(mf, I1, I2, B, (cx, cy, 1, 1), want=("stats",))
        assert st[0] == int(ok), (cx, cy, ok)
    E = extreme_grid(W0, H0, 11)
    out, _ = _assert_device_equals_host(bbme, mf, I1, I2, E, None, "int16 extremes")
    assert out.min() == -32768 and out.max() == 32767
    noise = rng.integers(0, 256, size=(2, H0, W0)).astype(np.uint8)            # costs in their upper range
    _assert_device_equals_host(bbme, mf, noise[0], noise[1], G, None, "noise")
    _assert_device_equals_host(bbme, mf, np.zeros_like(I1), np.full_like(I1, 255), np.zeros_like(G), None, "ceiling")
    # refusals: pitch below a row, a window outside the cells, an output on top of the input grid
    tg = _cuda(G)
    t1, t2 = _cuda(I1), _cuda(I2)
    for kw in (dict(out=tg), dict(out=torch.zeros((CH, CW, 2), dtype=torch.int16, device="cuda"), window=(0, 0, CW + 1, 1)),
               dict()):
        with pytest.raises(bbme.BbmeError) as e:
            mf.cells_subpel_device(t1, t2, tg, **kw)
        assert e.value.status == -1, kw
    mf.close()


CONTEXT_CASES = [(200, 120, [20, 20], [8, 8], 5), (128, 96, [30, 30, 30], [16, 16, 16], 9)]


@pytest.mark.parametrize("w,h,search,block,mm", CONTEXT_CASES)
def test_own_fields_both_directions_and_state(bbme, w, h, search, block, mm):
    f1, f2, _ = bbme.synth_pair(w, h, 40 + w, max_motion=mm)
    mf = bbme.MF(f1, f2, search, block)
    I1, I2 = mf.get_level_planes(0)
    # after a plain estimate: forward works, backward has no field
    flow = mf.calcMotionBlockMatching()
    cells = mf.get_cells()
    exp_f = _host(bbme, I1, I2, cells)
    assert np.array_equal(mf.subpel_cells("forward"), exp_f[0])
    assert _stats(mf.subpel_stats("forward", "all")) == exp_f[1]
    for call in (lambda: mf.subpel_cells("backward"), lambda: mf.subpel_stats("backward"), lambda: mf.subpel_flow("backward")):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == -7
    assert np.array_equal(mf.get_cells(), cells) and np.array_equal(mf.get_flow(), flow)
    # after a bidirectional estimate: both, the backward one on the exchanged planes
    mf.estimate_bidirectional_async()
    bwd = mf.get_backward_cells()
    assert np.array_equal(mf.get_cells(), cells)
    exp_b = _host(bbme, I2, I1, bwd)
    win = mf.default_cell_window()
    for _ in range(2):
        assert np.array_equal(mf.subpel_cells("forward"), exp_f[0])
        assert np.array_equal(mf.subpel_cells("backward"), exp_b[0])
        assert _stats(mf.subpel_stats("forward")) == _host(bbme, I1, I2, cells, win)[1]
        assert _stats(mf.subpel_stats("backward", "all")) == exp_b[1]
    assert exp_f[1][1] > 0 and exp_b[1][1] > 0 and not np.array_equal(exp_f[0], 4 * cells)
    # the field: every pixel its cell's vector / 4
    for which, q4 in (("forward", exp_f[0]), ("backward", exp_b[0])):
        assert np.array_equal(mf.subpel_flow(which), cells_to_field(q4, mf.padding_x, mf.padding_y, w, h, 4))
    # state: cells, backward cells, the flow, and what a second estimate gives
    assert np.array_equal(mf.get_cells(), cells) and np.array_equal(mf.get_backward_cells(), bwd)
    assert np.array_equal(mf.get_flow(), flow)
    assert np.array_equal(mf.calcMotionBlockMatching(), flow)
    assert np.array_equal(mf.subpel_cells("forward"), exp_f[0])
    with pytest.raises(bbme.BbmeError) as e:               # the estimate ended the pair of fields
        mf.subpel_cells("backward")
    assert e.value.status == -7
    # direction BACKWARD: the planes exchange as for every plane-reading call
    mf.set_direction(True)
    mf.calcMotionBlockMatching()
    assert np.array_equal(mf.get_cells(), bwd)
    assert np.array_equal(mf.subpel_cells("forward"), exp_b[0])
    with pytest.raises(bbme.BbmeError) as e:
        mf.subpel_cells(2)
    assert e.value.status == -1
    mf.close()


def test_before_any_estimate(bbme):
    f1, f2, _ = bbme.synth_pair(128, 96, 3, max_motion=4)
    mf = bbme.MF(f1, f2, [20, 20], [8, 8])
    for call in (lambda: mf.subpel_cells(), lambda: mf.subpel_stats(), lambda: mf.subpel_flow()):
        with pytest.raises(bbme.BbmeError) as e:
            call()
        assert e.value.status == -7
    mf.close()


def test_batch_and_chain(bbme):
    w, h, search, block = 136, 104, [20, 20], [8, 8]
    frames = bbme.synth_video(w, h, 3, 21, max_motion=4)
    pairs = [(frames[0], frames[1]), (frames[1], frames[2])]
    single = []
    for a, b in pairs:
        mf = bbme.MF(a, b, search, block)
        mf.estimate_bidirectional_async()
        single.append({"f": mf.subpel_cells("forward"), "b": mf.subpel_cells("backward"), "ff": mf.subpel_flow("forward"),
                       "sf": mf.subpel_stats("forward"), "sb": mf.subpel_stats("backward", "all")})
        assert not np.array_equal(single[-1]["f"], 4 * mf.get_cells())
        mf.close()
    batch = bbme.MFBatch(pairs, search, block)
    chain = bbme.MFChain(frames, search, block)
    for ctx in (batch, chain):
        ctx.estimate_bidirectional_async()
        for p in (1, 0):
            assert np.array_equal(ctx.get_pair_subpel_cells(p, "forward"), single[p]["f"]), p
            assert np.array_equal(ctx.get_pair_subpel_cells(p, "backward"), single[p]["b"]), p
            assert np.array_equal(ctx.get_pair_subpel_flow(p, "forward"), single[p]["ff"]), p
        assert ctx.subpel_stats_all("forward") == [s["sf"] for s in single]
        assert ctx.subpel_stats_all("backward", "all") == [s["sb"] for s in single]
        ctx.close()


def test_upsampled_context_divides_by_16(bbme):
    w, h = 48, 40
    f1, f2, _ = bbme.synth_pair(w, h, 8, max_motion=2)
    mf = bbme.MF(f1, f2, [24, 24], [8, 8], upsample=4)
    mf.estimate_bidirectional_async()
    I1, I2 = mf.get_level_planes(0)
    assert I1.shape == (mf.padded_height, mf.padded_width) and mf.padded_width >= 4 * w
    for which, a, b, cells in (("forward", I1, I2, mf.get_cells()), ("backward", I2, I1, mf.get_backward_cells())):
        q4 = _host(bbme, a, b, cells)[0]
        assert np.array_equal(mf.subpel_cells(which), q4)
        ys, xs = np.mgrid[0:h, 0:w]
        exp = q4[(mf.padding_y + 4 * ys) >> 1, (mf.padding_x + 4 * xs) >> 1].astype(np.float32) / np.float32(16)
        got = mf.subpel_flow(which)
        assert got.shape == (h, w, 2) and np.array_equal(got, exp)
    mf.close()


def test_pipelined_frames_return_quarter_pel_cells(bbme):
    from blockbasedmotionestimation_amd import sequence
    w, h, search, block = 136, 104, [20, 20], [8, 8]
    frames = bbme.synth_video(w, h, 4, 33, max_motion=4)
    got = sequence.estimate_frames_pipelined(frames, search, block, device=0, in_flight=2, batch=2, subpel=True)
    plain = sequence.estimate_frames_pipelined(frames, search, block, device=0, in_flight=2, batch=2)
    assert len(got) == len(plain) == 3
    for p in range(3):
        mf = bbme.MF(frames[p], frames[p + 1], search, block)
        mf.calcMotionBlockMatching()
        assert np.array_equal(got[p], mf.subpel_cells()), p
        assert np.array_equal(plain[p], mf.get_subsampled_flow(1)), p
        mf.close()


def test_cli_writes_the_refined_field(bbme, venus_flo, tmp_path):
    """bbme_cli --no-upsample --subpel on the pair of the quality test (tests/test_subpel_cpu.py): the file is MF.subpel_flow's
    field, the EPE line is printed beside the integer field's, and without --subpel nothing changes."""
    from blockbasedmotionestimation_amd import build as _build
    fl = bbme.Flow()
    gt = fl.ReadFlowFile(venus_flo)
    f1, f2 = bbme.warp_pair_from_flow(gt)
    _write_pgm(tmp_path / "f1.pgm", f1)
    _write_pgm(tmp_path / "f2.pgm", f2)
    args = [_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm"), "--no-upsample", "--levels", "3", "--block", "8",
            "--search", "16", "--gt", venus_flo, "--out", str(tmp_path / "int.flo")]
    r = subprocess.run(args + ["--subpel", str(tmp_path / "sub.flo")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(f1, f2, [16] * 3, [8] * 3)
    mf.calcMotionBlockMatching()
    exp_int, exp_sub = mf.get_subsampled_flow(1), mf.subpel_flow()
    mf.close()
    fl.WriteFlowFile(exp_sub, str(tmp_path / "exp_sub.flo"))
    fl.WriteFlowFile(exp_int, str(tmp_path / "exp_int.flo"))
    assert (tmp_path / "sub.flo").read_bytes() == (tmp_path / "exp_sub.flo").read_bytes()
    assert (tmp_path / "int.flo").read_bytes() == (tmp_path / "exp_int.flo").read_bytes()
    epe_int, epe_sub = fl.CalculateMSE(gt, exp_int), fl.CalculateMSE(gt, exp_sub)
    assert ("Calculated MSE is %.9g\n" % epe_int) in r.stdout
    assert ("Calculated MSE after quarter-pel refinement is %.9g\n" % epe_sub) in r.stdout
    assert epe_sub <= 0.6 * epe_int and epe_sub <= 0.20              # the quality test's bounds, on the GPU's own field
    plain = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "quarter-pel" not in plain.stdout
    assert [l for l in plain.stdout.splitlines() if not l.startswith("Seconds")] == \
           [l for l in r.stdout.splitlines() if not l.startswith("Seconds") and "quarter-pel" not in l]


def test_two_megapixels(bbme):
    """1920 x 1088: 522 240 cells in 2 040 workgroups, byte offsets beyond 2^16 in both planes and a grid beyond 2^16 cells"""
    w, h = 1920, 1088
    f1, f2, motion = bbme.synth_pair(w, h, 5, max_motion=4)
    mf = bbme.MF(f1, f2, [24, 24], [16, 16])
    assert (mf.padded_width, mf.padded_height) == (w, h)
    CH, CW = mf.cells_shape
    rng = np.random.default_rng(1)
    G = (motion[::2, ::2] + rng.integers(-1, 2, size=(CH, CW, 2))).astype(np.int16)
    I1, I2 = mf.get_level_planes(0)
    _, st = _assert_device_equals_host(bbme, mf, I1, I2, G, None, "2 Mpixel")
    assert st[0] > 0.95 * CH * CW and st[1] > 0.5 * st[0]
    mf.close()
