"""The reference's x4 pipeline on the GPU (main_class.cpp:32-33, 58-70): original frames in (k_resize_x4_pad_run writes the
level-0 planes), the subsampled field out (k_subsample reads the 2x2-cell grid).  Everything must be byte for byte what the
host pipeline resize_x4 -> MF -> get_flow -> subsample_div4 gives.

The planes are also compared with the CPU oracle (resize_linear_x4, pad_zero, pyr_down) on content that tells a wrong filter weight
or truncation apart -- noise, 0 / 255 noise, a checkerboard of period 1, ramps, white -- and on the smallest sources there are:
one column, one row, rows shorter than the kernel's 8-byte window; through host frames, device frames with a pitch and the
frame runs of a chain context."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import HARD_CONTENTS, _write_pgm, hard_content

pytestmark = pytest.mark.gpu

REF = ([64] * 4, [32] * 4)                        # main_class.cpp:19-21
REF2 = ([32, 32, 42], [16, 16, 32])               # main_class.cpp:15-17
SMALL = ([30, 30], [16, 16])

# (source width, source height, (search, block)): odd and even sizes (pad_x % 4 = 2 and 0), widths not a multiple of 16,
# and the reference's two literal sets at the reference's frame size
PLANE_CASES = [(37, 29, SMALL), (40, 30, SMALL), (45, 22, SMALL), (38, 33, SMALL), (584, 388, REF), (584, 388, REF2)]


class _Dev:
    """A torch view of `nbytes` bytes of device memory the library owns."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 3}


def _fill_level0(mf, value):
    import torch
    mf.synchronize()
    w, h, _, _ = mf.level_geometry(0)
    for p in mf.level_planes_device(0):
        torch.as_tensor(_Dev(p, w * h), device="cuda").fill_(value)
    torch.cuda.synchronize()


def _pair(w, h, seed):
    import blockbasedmotionestimation_amd as bbme
    f1, f2, _ = bbme.synth_pair(w, h, seed, max_motion=3)
    return f1, f2


def _planes(mf):
    return [mf.get_level_planes(l) for l in range(mf.num_levels)]


@pytest.mark.parametrize("w,h,cfg", PLANE_CASES, ids=["%dx%d_%s" % (w, h, "ref" if c is REF else "ref2" if c is REF2 else "small")
                                                      for w, h, c in PLANE_CASES])
def test_x4_planes_equal_host_resize(bbme, w, h, cfg):
    import torch
    search, block = cfg
    f1, f2 = _pair(w, h, 1000 + w + h)
    host = bbme.MF(bbme.resize_x4(f1), bbme.resize_x4(f2), search, block)
    exp = _planes(host)
    mf = bbme.MF(f1, f2, search, block, upsample=4)
    assert (mf.orig_width, mf.orig_height, mf.source_width, mf.source_height) == (4 * w, 4 * h, w, h)
    assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == \
           (host.padded_width, host.padded_height, host.padding_x, host.padding_y)
    for l, (a, b) in enumerate(_planes(mf)):
        assert np.array_equal(a, exp[l][0]) and np.array_equal(b, exp[l][1]), "level %d" % l
    # a stale plane: every byte, borders included, must be written again
    g1, g2 = _pair(w, h, 2000 + w + h)
    host.set_frames(bbme.resize_x4(g1), bbme.resize_x4(g2))
    exp = _planes(host)
    _fill_level0(mf, 0xAB)
    mf.set_frames(g1, g2)
    for l, (a, b) in enumerate(_planes(mf)):
        assert np.array_equal(a, exp[l][0]) and np.array_equal(b, exp[l][1]), "host x4, level %d" % l
    # from HBM, rows further apart than the frame is wide
    _fill_level0(mf, 0xAB)
    dev = []
    for f in (g1, g2):
        big = torch.full((h, w + 13), 7, dtype=torch.uint8, device="cuda")
        big[:, :w] = torch.from_numpy(f).cuda()
        dev.append(big[:, :w])
    assert dev[0].stride(0) == w + 13
    mf.set_frames_device(*dev)
    for l, (a, b) in enumerate(_planes(mf)):
        assert np.array_equal(a, exp[l][0]) and np.array_equal(b, exp[l][1]), "device x4, level %d" % l
    mf.close()
    host.close()


# (source width, source height, search, block, (padded width, padded height, pad_x, pad_y) of the x4 frame)
HARD_SOURCES = [(1, 1, [2], [2], (4, 4, 0, 0)),                   # one source pixel: sw - 1 == 0 and sh == 1, every tap clamped
                (2, 1, [2], [2], (8, 4, 0, 0)),                   # one row
                (1, 2, [2], [2], (4, 8, 0, 0)),                   # one column
                (3, 2, [2], [2], (12, 8, 0, 0)),                  # a row shorter than the 8 bytes a thread gathers
                (5, 3, [8], [8], (24, 16, 2, 2)),                 # padded both ways, the row's last chunk is half a chunk
                (9, 7, [4, 4], [4, 4], (40, 32, 2, 2)),           # two levels: a pyrDown row of five threads
                (45, 22) + SMALL + ((192, 96, 6, 4),)]


def _oracle_planes(oracle, frame, pad_x, pad_y, levels):
    planes = [oracle.pad_zero(oracle.resize_linear_x4(frame), pad_x, pad_y)]
    for _ in range(levels - 1):
        planes.append(oracle.pyr_down(planes[-1]))
    return planes


@pytest.mark.parametrize("w,h,search,block,plan", HARD_SOURCES, ids=["%dx%d" % c[:2] for c in HARD_SOURCES])
def test_x4_planes_of_hard_content_equal_the_oracle(bbme, oracle, w, h, search, block, plan):
    """Every plane of every level against oracle.pad_zero(oracle.resize_linear_x4(frame)) and its pyr_down cascade -- not
    against a second context of this library.  The contexts are re-used from content to content, so every byte of a plane has
    to be written again each time."""
    import torch
    assert bbme.plan_padding(4 * w, 4 * h, search, block) == plan
    L = len(block)
    frames = [hard_content(name, h, w, seed=7) for name in HARD_CONTENTS]
    exp = [_oracle_planes(oracle, f, plan[2], plan[3], L) for f in frames]
    assert exp[0][0].shape == (plan[1], plan[0])
    n = len(frames)
    mf = chain = None
    for k in range(n):
        a, b = k, (k + 1) % n
        # host frames
        if mf is None:
            mf = bbme.MF(frames[a], frames[b], search, block, upsample=4)
            assert (mf.padded_width, mf.padded_height, mf.padding_x, mf.padding_y) == plan
        else:
            mf.set_frames(frames[a], frames[b])
        for l in range(L):
            p1, p2 = mf.get_level_planes(l)
            assert np.array_equal(p1, exp[a][l]) and np.array_equal(p2, exp[b][l]), ("host", HARD_CONTENTS[a], l)
        # device frames, rows further apart than the frame is wide; the other order, so that both planes change
        dev = []
        for f in (frames[b], frames[a]):
            big = torch.full((h, w + 13), 7, dtype=torch.uint8, device="cuda")
            big[:, :w] = torch.from_numpy(f).cuda()
            dev.append(big[:, :w])
        mf.set_frames_device(*dev)
        for l in range(L):
            p1, p2 = mf.get_level_planes(l)
            assert np.array_equal(p1, exp[b][l]) and np.array_equal(p2, exp[a][l]), ("device", HARD_CONTENTS[a], l)
    mf.close()
    # a chain of two pairs: three frames per run, the frame as a grid dimension (k_resize_x4_pad_run, k_pyr_down4_run)
    for first in (0, 3, 1):
        run = [(first + i) % n for i in range(3)]
        if chain is None:
            chain = bbme.MFChain([frames[i] for i in run], search, block, upsample=4)
            assert chain.batch == 2 and chain.slots == 3
        else:
            chain.set_frame_run(0, [frames[i] for i in run])
        for slot, i in enumerate(run):
            for l in range(L):
                assert np.array_equal(chain.get_slot_plane(l, slot), exp[i][l]), ("chain", HARD_CONTENTS[i], slot, l)
    chain.close()
    # frames in HBM; then a run with a pitch into the last two slots only: the first keeps its planes
    chain = bbme.MFChain([torch.from_numpy(frames[i]).cuda() for i in (2, 3, 5)], search, block, frames_on_device=True, upsample=4)
    dev = []
    for i in (4, 0):
        big = torch.full((h, w + 5), 9, dtype=torch.uint8, device="cuda")
        big[:, :w] = torch.from_numpy(frames[i]).cuda()
        dev.append(big[:, :w])
    chain.set_frame_run(1, dev)
    for slot, i in enumerate((2, 4, 0)):
        for l in range(L):
            assert np.array_equal(chain.get_slot_plane(l, slot), exp[i][l]), ("chain, device run", HARD_CONTENTS[i], slot, l)
    chain.close()


@pytest.fixture(scope="module")
def venus(bbme, venus_flo):
    """The reference's pipeline on the Venus-warped pair, host side and x4 side."""
    gt = bbme.Flow().ReadFlowFile(venus_flo)
    h, w = gt.shape[:2]
    f1, f2 = bbme.warp_pair_from_flow(gt)
    host = bbme.MF(bbme.resize_x4(f1), bbme.resize_x4(f2), *REF)
    flow = host.calcMotionBlockMatching()
    cells = host.get_cells()
    sub = bbme.subsample_div4(flow, host.padding_x, host.padding_y, w, h)
    epe = bbme.Flow().CalculateMSE(gt, sub)
    host.close()
    mf = bbme.MF(f1, f2, *REF, upsample=4)
    mf.estimate_async()
    yield dict(gt=gt, f1=f1, f2=f2, flow=flow, cells=cells, sub=sub, epe=epe, mf=mf, w=w, h=h)
    mf.close()


def test_x4_fields_equal_host_pipeline(bbme, venus):
    assert np.array_equal(venus["mf"].get_cells(), venus["cells"])
    f1, f2 = _pair(160, 120, 77)
    search, block = [30, 30, 30], [16, 16, 16]
    host = bbme.MF(bbme.resize_x4(f1), bbme.resize_x4(f2), search, block)
    host.estimate_async()
    mf = bbme.MF(f1, f2, search, block, upsample=4)
    mf.estimate_async()
    assert np.array_equal(mf.get_cells(), host.get_cells())
    assert np.array_equal(mf.get_flow(), host.get_flow())
    mf.close()
    host.close()


def test_subsampled_output(bbme, venus):
    import torch
    mf, flow, w, h = venus["mf"], venus["flow"], venus["w"], venus["h"]
    px, py, W, H = mf.padding_x, mf.padding_y, mf.orig_width, mf.orig_height
    sub = mf.get_subsampled_flow()
    assert sub.shape == (h, w, 2) and sub.dtype == np.float32
    assert np.array_equal(sub, venus["sub"])
    assert np.array_equal(mf.get_subsampled_flow(4), venus["sub"])
    assert np.array_equal(mf.get_subsampled_flow(1), flow[py:py + H, px:px + W])
    assert np.array_equal(mf.get_subsampled_flow(3), flow[py:py + H:3, px:px + W:3] / np.float32(3))
    # exactly the host pipeline's EPE
    assert bbme.Flow().CalculateMSE(venus["gt"], sub) == venus["epe"]
    # device entry point: caller's pitch, caller's stream
    s = torch.cuda.Stream()
    big = torch.full((h, w + 9, 2), -7.0, dtype=torch.float32, device="cuda")
    mf.subsampled_flow_device(big[:, :w], 4, s.cuda_stream)
    s.synchronize()
    got = big.cpu().numpy()
    assert np.array_equal(got[:, :w], venus["sub"])
    assert (got[:, w:] == -7.0).all()
    big1 = torch.full((H, W + 3, 2), -7.0, dtype=torch.float32, device="cuda")
    mf.subsampled_flow_device(big1[:, :W], 1)
    mf.synchronize()
    got = big1.cpu().numpy()
    assert np.array_equal(got[:, :W], flow[py:py + H, px:px + W]) and (got[:, W:] == -7.0).all()


def test_batch_pairs_equal_single_contexts(bbme):
    search, block = [30, 30, 30], [16, 16, 16]
    pairs = [_pair(96, 72, 300 + i) for i in range(3)]
    mb = bbme.MFBatch(pairs, search, block, upsample=4)
    assert (mb.orig_width, mb.orig_height, mb.source_width, mb.source_height) == (384, 288, 96, 72)
    mb.estimate_async()

    def single(p):
        mf = bbme.MF(p[0], p[1], search, block, upsample=4)
        r = mf.calcMotionBlockMatchingSubsampled()
        mf.close()
        return r

    exp = [single(p) for p in pairs]
    got = [mb.get_pair_subsampled_flow(i) for i in range(3)]
    for i in range(3):
        assert got[i].shape == (72, 96, 2)
        assert np.array_equal(got[i], exp[i]), "pair %d" % i
    new = _pair(96, 72, 999)
    mb.set_pair(1, *new)
    mb.estimate_async()
    assert np.array_equal(mb.get_pair_subsampled_flow(0), exp[0])
    assert np.array_equal(mb.get_pair_subsampled_flow(2), exp[2])
    exp1 = single(new)
    assert np.array_equal(mb.get_pair_subsampled_flow(1), exp1)
    # the same pair from HBM
    import torch
    mb.set_pair_device(1, torch.from_numpy(pairs[1][0]).cuda(), torch.from_numpy(pairs[1][1]).cuda())
    mb.estimate_async()
    for i in range(3):
        assert np.array_equal(mb.get_pair_subsampled_flow(i), exp[i]), "pair %d after the device refill" % i
    mb.close()


def test_x4_errors(bbme):
    from blockbasedmotionestimation_amd import _capi
    L = _capi.lib()
    search, block = [30, 30], [16, 16]
    f1, f2 = _pair(40, 30, 5)
    # a context whose frame is not a multiple of 4
    odd = bbme.MF(*_pair(150, 118, 6), search, block)
    z = np.zeros((30, 38), np.uint8)
    assert L.bbme_set_frames_host_x4(odd._ctx, 0, z.ctypes.data, z.ctypes.data, 38) == _capi.ERR_INVALID
    assert L.bbme_set_frames_host_x4_async(odd._ctx, 0, z.ctypes.data, z.ctypes.data, 38) == _capi.ERR_INVALID
    assert L.bbme_set_frames_device_x4(odd._ctx, 0, odd.flow_device_ptr(), odd.flow_device_ptr(), 38) == _capi.ERR_INVALID
    odd.close()
    mf = bbme.MF(f1, f2, search, block, upsample=4)
    # pitch < width / 4
    assert L.bbme_set_frames_host_x4(mf._ctx, 0, f1.ctypes.data, f2.ctypes.data, 39) == _capi.ERR_INVALID
    assert L.bbme_set_frames_host_x4(mf._ctx, 1, f1.ctypes.data, f2.ctypes.data, 40) == _capi.ERR_INVALID
    # nothing estimated yet
    with pytest.raises(bbme.BbmeError) as e:
        mf.get_subsampled_flow()
    assert e.value.status == _capi.ERR_STATE
    out = np.zeros((30, 40, 2), np.float32)
    assert L.bbme_get_subsampled_flow_host(mf._ctx, 0, 4, out.ctypes.data) == _capi.ERR_STATE
    assert L.bbme_subsampled_flow_device(mf._ctx, 0, 4, C.c_void_p(mf.flow_device_ptr()), 40, None) == _capi.ERR_STATE
    mf.estimate_async()
    assert L.bbme_get_subsampled_flow_host(mf._ctx, 0, 0, out.ctypes.data) == _capi.ERR_INVALID
    assert L.bbme_get_subsampled_flow_host(mf._ctx, 0, -4, out.ctypes.data) == _capi.ERR_INVALID
    assert L.bbme_subsampled_flow_device(mf._ctx, 0, 0, C.c_void_p(mf.flow_device_ptr()), 40, None) == _capi.ERR_INVALID
    assert L.bbme_subsampled_flow_device(mf._ctx, 0, 4, C.c_void_p(mf.flow_device_ptr()), 39, None) == _capi.ERR_INVALID
    with pytest.raises(bbme.BbmeError) as e:
        mf.get_subsampled_flow(0)
    assert e.value.status == _capi.ERR_INVALID
    assert L.bbme_get_subsampled_flow_host(mf._ctx, 0, 4, out.ctypes.data) == _capi.OK
    mf.close()


def test_cli_output_equals_host_pipeline(bbme, venus, venus_flo, tmp_path):
    from blockbasedmotionestimation_amd import build as _build
    _write_pgm(tmp_path / "f1.pgm", venus["f1"])
    _write_pgm(tmp_path / "f2.pgm", venus["f2"])
    r = subprocess.run([_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm"), "--out", str(tmp_path / "a.flo"),
                        "--color", str(tmp_path / "a.ppm"), "--gt", venus_flo], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    fl = bbme.Flow()
    fl.WriteFlowFile(venus["sub"], str(tmp_path / "b.flo"))
    fl.ShowImage(fl.MotionToColor(venus["sub"], verbose=False), str(tmp_path / "b.ppm"))
    assert (tmp_path / "a.flo").read_bytes() == (tmp_path / "b.flo").read_bytes()
    assert (tmp_path / "a.ppm").read_bytes() == (tmp_path / "b.ppm").read_bytes()
    assert ("Calculated MSE is %.9g\n" % venus["epe"]) in r.stdout
    # --no-upsample: the unpadded window of the full-resolution field
    h, w = venus["h"], venus["w"]
    r = subprocess.run([_build.CLI, str(tmp_path / "f1.pgm"), str(tmp_path / "f2.pgm"), "--out", str(tmp_path / "c.flo"),
                        "--no-upsample", "--levels", "3", "--block", "16", "--search", "30"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    mf = bbme.MF(venus["f1"], venus["f2"], [30] * 3, [16] * 3)
    flow = mf.calcMotionBlockMatching()
    fl.WriteFlowFile(np.ascontiguousarray(flow[mf.padding_y:mf.padding_y + h, mf.padding_x:mf.padding_x + w]),
                     str(tmp_path / "d.flo"))
    mf.close()
    assert (tmp_path / "c.flo").read_bytes() == (tmp_path / "d.flo").read_bytes()
    assert os.path.getsize(tmp_path / "c.flo") == 12 + 8 * w * h
