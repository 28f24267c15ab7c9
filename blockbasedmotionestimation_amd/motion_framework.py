"""Python mirror of the reference's MF class (motion_framework.h:9-54) over the C-ABI.

    mf = MF(image1, image2, search_size, block_size, num_levels)   # MF::MF, motion_framework.cpp:4-111
    flow = mf.calcMotionBlockMatching()                             # :113-219 -> (H_pad, W_pad, 2) float32
    mf.padded_height, mf.padded_width, mf.padding_x, mf.padding_y   # public fields :16-19

    mf = MF(image1, image2, search_size, block_size, upsample=4)   # the original frames of main_class.cpp:32-33
    sub = mf.calcMotionBlockMatchingSubsampled()                    # :58-70 on the GPU -> (h, w, 2) float32
    mc = mf.draw_MVimage(level=0, block=2)                          # :887-905 on the GPU -> (H_pad, W_pad) uint8
    err = mf.compensation_error()                                   # its sse / sad / pixels / skipped / mse / psnr

Argument meaning and order follow the reference: arrays are indexed [0] = finest level,
search_size is the window side length.  Errors the reference reports with assert / exit(1)
raise BbmeError here.  All arithmetic runs in the HIP kernels of libbbme.so.
"""
import ctypes as C
import math

import numpy as np

from . import _capi


DIR_FORWARD, DIR_BACKWARD = 0, 1                           # bbme_set_direction, `which` of the consistency calls
FB_CONSISTENT, FB_INCONSISTENT, FB_OUTSIDE = 0, 1, 2      # classes of a consistency mask
INTERPOLATION_STAT_KEYS = ("forward", "backward", "zero", "cost")      # the hypothesis a cell selected (0, 1, 2), their SADs
# cells with w_k > 0 for P1, N1, P2, N2, sum of all weights, sum |out - C|
WIDE_STAT_KEYS = ("prev1_cells", "next1_cells", "prev2_cells", "next2_cells", "weight", "change")
COMPOSE_STAT_KEYS = ("clamped", "saturated")    # cells whose target cell was clamped into the grid, cells that saturated
TEMPORAL_STAT_KEYS = ("prev_cells", "next_cells", "weight", "change")  # cells with wP > 0, with wN > 0, sum of weights, sum |out - C|


def _check_upsample(upsample):
    if upsample not in (1, 4):
        raise _capi.BbmeError(_capi.ERR_INVALID, "upsample must be 1 or 4, not %r" % (upsample,))
    return upsample


def _ptr(t):
    """The address of a CUDA tensor's or a numpy array's data for a C entry point; None is the null pointer."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)


def _ptr4(items):
    """Four addresses as the pointer array of a C entry point (the wide temporal filter's planes and grids); None is null."""
    return (C.c_void_p * 4)(*[_ptr(t).value for t in items])


def _window(window):
    """(x0, y0, w, h) as the four ints of a C entry point; None stays None (the call's whole plane or grid)."""
    return None if window is None else (C.c_int * 4)(*[int(v) for v in window])


def _host_out(out, shape, dtype, what):
    """A host result array: a new one, or the caller's when it has that shape and type and is C-contiguous."""
    if out is None:
        return np.empty(shape, dtype)
    if out.shape != shape or out.dtype != dtype or not out.flags.c_contiguous:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a C-contiguous %s array of shape %s" % (what, np.dtype(dtype).name, shape))
    return out


class MF:
    """upsample=4: image1 / image2 are the original frames of the reference's pipeline, which up-samples them x4 before
    MF::MF (main_class.cpp:32-33).  The context is created at the up-sampled size (orig_width / orig_height keep meaning
    "the frame MF sees", source_width / source_height are the frames passed in) and the up-sampling runs on the GPU
    (bbme_set_frames_host_x4 / bbme_set_frames_device_x4): the planes are byte for byte those of MF(resize_x4(image1),
    resize_x4(image2), ...).  set_frames / set_frames_device then take frames of the source size too."""

    def __init__(self, image1, image2, search_size, block_size, num_levels=None, device=0,
                 frames_on_device=False, upsample=1):
        self.upsample = _check_upsample(upsample)
        if num_levels is None:
            num_levels = len(block_size)
        if num_levels <= 0:
            raise _capi.BbmeError(_capi.ERR_INVALID, "num_levels must be > 0")       # assert :7
        search_size = list(search_size)[:num_levels]
        block_size = list(block_size)[:num_levels]
        self._ctx = C.c_void_p()
        self._lib = _capi.lib()
        self.device = device
        self._torch_frames = None
        if frames_on_device:
            import torch
            if tuple(image1.shape) != tuple(image2.shape) or not _is_frame_shape(tuple(image1.shape)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "image1.size() != image2.size()")
            h, w = image1.shape[:2]
        else:
            image1 = np.ascontiguousarray(image1, dtype=np.uint8)
            image2 = np.ascontiguousarray(image2, dtype=np.uint8)
            if not _is_frame_shape(image1.shape) or image1.shape != image2.shape:       # assert :8
                raise _capi.BbmeError(_capi.ERR_INVALID, "image1.size() != image2.size()")
            h, w = image1.shape[:2]
        self.source_height, self.source_width = h, w
        self.orig_height, self.orig_width = h * upsample, w * upsample
        self.params = _capi.make_params(search_size, block_size)
        _capi.check(self._lib.bbme_create(C.byref(self.params), self.orig_width, self.orig_height, device, C.byref(self._ctx)))
        pw, ph, px, py = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _capi.check(self._lib.bbme_get_geometry(self._ctx, C.byref(pw), C.byref(ph), C.byref(px), C.byref(py)))
        self.padded_width, self.padded_height = pw.value, ph.value
        self.padding_x, self.padding_y = px.value, py.value
        self.num_levels = num_levels
        if frames_on_device:
            self.set_frames_device(image1, image2)
        else:
            self.set_frames(image1, image2)

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.bbme_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- inputs ---------------------------------------------------------------------------
    def _host_frames(self, image1, image2):
        image1 = np.ascontiguousarray(image1, dtype=np.uint8)
        image2 = np.ascontiguousarray(image2, dtype=np.uint8)
        if image1.shape not in self._frame_shapes() or image2.shape != image1.shape:
            raise _capi.BbmeError(_capi.ERR_INVALID, "frames must keep the size the context was created for")
        return image1, image2

    def _frame_shapes(self):
        """The shapes a frame of this context may have: grey (H, W), or colour (H, W, 3) in B,G,R order (the luma rule of
        include/bbme.h; not on an upsample=4 context)."""
        grey = (self.source_height, self.source_width)
        return (grey,) if self.upsample == 4 else (grey, grey + (3,))

    def _set_host_pair(self, pair, image1, image2):
        image1, image2 = self._host_frames(image1, image2)
        if image1.ndim == 3:
            _capi.check(self._lib.bbme_set_frames_host_bgr(self._ctx, pair, image1.ctypes.data, image2.ctypes.data,
                                                           3 * self.source_width))
        elif self.upsample == 4:
            _capi.check(self._lib.bbme_set_frames_host_x4(self._ctx, pair, image1.ctypes.data, image2.ctypes.data,
                                                          self.source_width))
        else:
            _capi.check(self._lib.bbme_set_frames_host_pair(self._ctx, pair, image1.ctypes.data, image2.ctypes.data,
                                                            self.source_width))

    def _set_device_pair(self, pair, image1, image2):
        self._check_device_frames(image1, image2)
        # the tensors may still be being written by work on torch's current stream: order the context's stream behind it
        import torch
        _capi.check(self._lib.bbme_wait_for_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(image1.device).cuda_stream)))
        setter = self._lib.bbme_set_frames_device_x4 if self.upsample == 4 else self._lib.bbme_set_frames_device_pair
        if image1.dim() == 3:
            setter = self._lib.bbme_set_frames_device_bgr
        _capi.check(setter(self._ctx, pair, image1.data_ptr(), image2.data_ptr(), image1.stride(0)))

    def set_frames(self, image1, image2):
        """A new pair of the same size into this context (host arrays): what a second MF::MF would do,
        without re-allocating the level state or re-capturing the launch graph."""
        self._set_host_pair(0, image1, image2)

    def _check_device_frames(self, image1, image2):
        """The padding kernel reads source_height x pitch bytes behind each pointer: a tensor of any other shape must be
        refused here (the C-ABI sees only a pointer and a pitch)."""
        import torch
        for t in (image1, image2):
            if not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) in self._frame_shapes() and t.shape == image1.shape):
                raise _capi.BbmeError(_capi.ERR_INVALID, "device frames must be uint8 CUDA tensors of %d x %d, or %d x %d x 3 in "
                                      "B,G,R order (the size the context was created for)"
                                      % (self.source_height, self.source_width, self.source_height, self.source_width))
        if not (_packed_pixels(image1) and _packed_pixels(image2)) or image1.stride(0) != image2.stride(0):
            raise _capi.BbmeError(_capi.ERR_INVALID, "device frames must have packed pixels and a common row pitch")

    def _behind_torch(self, *tensors):
        """torch tensors handed to a *_device call may still be being written (a fill, an upload) or read by work on torch's
        current stream, which nothing orders against the context's non-blocking stream: order the context's stream behind it,
        as the frame setters do.  A caller's stream is ordered behind the context's by the library, so it is covered too.  No
        host wait."""
        import torch
        for dev in {t.device for t in tensors if t is not None}:
            _capi.check(self._lib.bbme_wait_for_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def set_frames_device(self, image1, image2):
        """Frames already in HBM (torch uint8 CUDA tensors, H x W of the source size): (x4 up-sampling,) padding and
        pyramid on the GPU."""
        self._set_device_pair(0, image1, image2)
        self._torch_frames = (image1, image2)

    def set_search_mode(self, raster):
        """False: find_min_block_spiral (the reference's live search); True: the raster find_min_block (:246-294)."""
        _capi.check(self._lib.bbme_set_search_mode(self._ctx, 1 if raster else 0))

    def set_regularizer_mode(self, jacobi):
        """False: the reference's in-place raster sweep, bit for bit.  True: opt-in Jacobi sweeps (not the reference's field)."""
        _capi.check(self._lib.bbme_set_regularizer_mode(self._ctx, 1 if jacobi else 0))

    def set_speculation(self, enabled):
        """Speculative search of the next finer level beside a level's late sweeps (bbme_set_speculation); same result."""
        _capi.check(self._lib.bbme_set_speculation(self._ctx, int(bool(enabled))))

    def set_relaxation(self, enabled):
        """Scheduling only (same field): the relaxation launches in front of the solver on large grids of small blocks.
        Turn them off, like the speculation, when several pairs are in flight on the GPU."""
        _capi.check(self._lib.bbme_set_relaxation(self._ctx, 1 if enabled else 0))

    def set_stream(self, hip_stream_handle):
        _capi.check(self._lib.bbme_set_stream(self._ctx, C.c_void_p(hip_stream_handle)))

    def level_geometry(self, level):
        w, h, b, s = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _capi.check(self._lib.bbme_level_geometry(self._ctx, level, C.byref(w), C.byref(h), C.byref(b), C.byref(s)))
        return w.value, h.value, b.value, s.value

    def set_level_planes(self, level, image1, image2):
        w, h, _, _ = self.level_geometry(level)
        image1 = np.ascontiguousarray(image1, np.uint8)
        image2 = np.ascontiguousarray(image2, np.uint8)
        assert image1.shape == (h, w) and image2.shape == (h, w)
        _capi.check(self._lib.bbme_set_level_planes_host(self._ctx, level, image1.ctypes.data, image2.ctypes.data))

    def level_planes_device(self, level):
        """Device pointers of the level's two padded planes (pitch = level width) for filling or inspecting them in place
        (bbme_level_planes_device).  After an in-place refill the next stage call at the level must be stage_search or
        stage_set_mvs; estimate() needs nothing."""
        d1, d2 = C.c_void_p(), C.c_void_p()
        _capi.check(self._lib.bbme_level_planes_device(self._ctx, level, C.byref(d1), C.byref(d2)))
        return d1.value, d2.value

    def get_level_planes(self, level):
        w, h, _, _ = self.level_geometry(level)
        a = np.empty((h, w), np.uint8)
        b = np.empty((h, w), np.uint8)
        _capi.check(self._lib.bbme_get_level_planes_host(self._ctx, level, a.ctypes.data, b.ctypes.data))
        return a, b

    # -- the hot path ---------------------------------------------------------------------
    def estimate_async(self):
        """Enqueue MF::calcMotionBlockMatching on the context's stream; no host wait."""
        _capi.check(self._lib.bbme_estimate(self._ctx))

    def synchronize(self):
        _capi.check(self._lib.bbme_synchronize(self._ctx))

    def get_flow(self, out=None):
        """The dense padded field; `out` may be a preallocated C-contiguous float32 array of that shape, e.g. a view
        of pinned memory (the 66.8 MB of a 4K field download about three times faster into pinned memory)."""
        shape = (self.padded_height, self.padded_width, 2)
        out = _host_out(out, shape, np.float32, "get_flow")
        _capi.check(self._lib.bbme_get_flow_host(self._ctx, out.ctypes.data))
        return out

    def subsampled_shape(self, scale=None):
        """(rows, cols, 2) of the subsampled field: ceil(orig / scale); scale defaults to upsample."""
        scale = self.upsample if scale is None else int(scale)
        if scale < 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "scale must be >= 1")
        return (-(-self.orig_height // scale), -(-self.orig_width // scale), 2)

    def _get_subsampled(self, pair, scale, out, what):
        shape = self.subsampled_shape(scale)
        scale = self.upsample if scale is None else int(scale)
        out = _host_out(out, shape, np.float32, what)
        _capi.check(self._lib.bbme_get_subsampled_flow_host(self._ctx, pair, scale, out.ctypes.data))
        return out

    def get_subsampled_flow(self, scale=None, out=None):
        """The driver's subsampling (main_class.cpp:58-70) on the GPU: the field of the unpadded frame at every `scale`-th
        pixel, divided by `scale` (default: upsample, i.e. the source frame's size) -> (rows, cols, 2) float32.  scale 4
        equals subsample_div4(get_flow(), ...), scale 1 the unpadded window of get_flow(); only that field is downloaded."""
        return self._get_subsampled(0, scale, out, "get_subsampled_flow")

    def subsampled_flow_device(self, out, scale=None, hip_stream_handle=None, pair=0):
        """The same into a float32 CUDA tensor of shape (rows, >= cols, 2) whose rows may be further apart than cols
        (a column slice of a wider tensor), on the given HIP stream (default: the context's), ordered behind the
        context's stream; no host wait."""
        scale = self.upsample if scale is None else int(scale)
        rows, cols, _ = self.subsampled_shape(scale)
        import torch
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.shape[0] == rows and out.shape[1] == cols
                and out.shape[2] == 2 and out.stride(2) == 1 and out.stride(1) == 2 and out.stride(0) % 2 == 0
                and out.stride(0) >= 2 * cols):
            raise _capi.BbmeError(_capi.ERR_INVALID, "subsampled_flow_device: out must be a float32 CUDA tensor of shape "
                                  "(%d, %d, 2) with unit pixel stride" % (rows, cols))
        self._behind_torch(out)
        _capi.check(self._lib.bbme_subsampled_flow_device(self._ctx, pair, scale, C.c_void_p(out.data_ptr()),
                                                          out.stride(0) // 2, C.c_void_p(hip_stream_handle or 0)))
        return out

    # -- motion compensation (MF::draw_MVimage, motion_framework.cpp:887-905; rule in include/bbme.h) -----------------
    def _get_motion_compensated(self, pair, level, block, fill, out, what):
        w, h, _, _ = self.level_geometry(level)
        out = _host_out(out, (h, w), np.uint8, what)
        _capi.check(self._lib.bbme_get_motion_compensated_host(self._ctx, pair, level, block, fill, out.ctypes.data))
        return out

    def draw_MVimage(self, level=0, block=2, fill=0, out=None):
        """MF::draw_MVimage from the level's current MV grid with block x block blocks: the padded (H_l, W_l) uint8 plane,
        every block a copy of image2 where its MV points, blocks whose source leaves the plane set to `fill`.  Level 0 with
        block 2 after calcMotionBlockMatching is the reference's "MC_imageL1" (:213-216)."""
        return self._get_motion_compensated(0, level, block, fill, out, "draw_MVimage")

    def motion_compensated_device(self, out, level=0, block=2, fill=0, hip_stream_handle=None, pair=0):
        """draw_MVimage into a uint8 CUDA tensor of shape (H_l, W_l) whose rows may be further apart than W_l (a column
        slice of a wider tensor), on the given HIP stream (default: the context's), ordered behind the context's stream;
        no host wait."""
        w, h, _, _ = self.level_geometry(level)
        import torch
        if not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and tuple(out.shape) == (h, w)
                and out.stride(1) == 1 and out.stride(0) >= w):
            raise _capi.BbmeError(_capi.ERR_INVALID, "motion_compensated_device: out must be a uint8 CUDA tensor of shape "
                                  "(%d, %d) with unit column stride" % (h, w))
        self._behind_torch(out)
        _capi.check(self._lib.bbme_motion_compensate_device(self._ctx, pair, level, block, fill, C.c_void_p(out.data_ptr()),
                                                            out.stride(0), C.c_void_p(hip_stream_handle or 0)))
        return out

    def _compensation_stats(self, level, block, window):
        if window is None and level == 0:
            window = (self.padding_x, self.padding_y, self.orig_width, self.orig_height)
        win = _window(window)
        pairs = getattr(self, "batch", 1)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_compensation_error(self._ctx, level, block, win, s))
        return [_residual_dict(s[4 * p:4 * p + 4]) for p in range(pairs)]

    def compensation_error(self, level=0, block=2, window=None):
        """Residual statistics of draw_MVimage(level, block) against image1 over window (x0, y0, w, h) of the level plane:
        dict(sse, sad, pixels, skipped, mse, psnr).  Skipped blocks count in neither sum; mse = sse / pixels and
        psnr = 10 log10(255^2 pixels / sse) (inf for sse = 0, nan when no pixel was compensated).  Default window: the
        unpadded frame at level 0, the whole plane at other levels."""
        return self._compensation_stats(level, block, window)[0]

    # -- direction, bidirectional estimate, forward-backward consistency (rules in include/bbme.h) ---------------------
    def set_direction(self, backward):
        """True: every estimate and result of this context as if image1 and image2 of every pair were exchanged (no plane is
        touched; the level grids become "nothing yet" until the next estimate).  False: forward, the default."""
        _capi.check(self._lib.bbme_set_direction(self._ctx, 1 if backward else 0))

    @property
    def direction(self):
        """DIR_FORWARD (0) or DIR_BACKWARD (1)."""
        d = C.c_int()
        _capi.check(self._lib.bbme_get_direction(self._ctx, C.byref(d)))
        return d.value

    def estimate_bidirectional_async(self):
        """Enqueue the backward estimate of every pair (its cells kept as the backward cells), then the forward estimate; no
        host wait.  Afterwards every getter is as after estimate_async() in direction forward."""
        _capi.check(self._lib.bbme_estimate_bidirectional(self._ctx))

    @property
    def cells_shape(self):
        return (self.padded_height // 2, self.padded_width // 2)

    def _get_backward_cells(self, pair, out, what):
        shape = self.cells_shape + (2,)
        out = _host_out(out, shape, np.int16, what)
        _capi.check(self._lib.bbme_get_backward_cells_host_pair(self._ctx, pair, out.ctypes.data))
        return out

    def get_backward_cells(self, out=None):
        """The 2x2-cell grid of the backward field after estimate_bidirectional_async() -> (CH, CW, 2) int16."""
        return self._get_backward_cells(0, out, "get_backward_cells")

    def backward_cells_device_ptr(self, pair=0):
        p = C.c_void_p()
        _capi.check(self._lib.bbme_backward_cells_device_pair(self._ctx, pair, C.byref(p)))
        return p.value

    def consistency(self, which="forward", tol=1, pair=0, out=None):
        """The forward-backward consistency mask of the context's two fields -> (CH, CW) uint8: 0 consistent, 1 inconsistent,
        2 target outside the plane.  which="forward": the mask on frame 1 (forward vector followed, backward vector read
        there); "backward": on frame 2."""
        shape = self.cells_shape
        out = _host_out(out, shape, np.uint8, "consistency")
        _capi.check(self._lib.bbme_get_consistency_host(self._ctx, pair, _which(which), int(tol), out.ctypes.data))
        return out

    def default_cell_window(self):
        """(cx0, cy0, cw, ch): the cells whose top-left pixel lies in the unpadded frame."""
        x0, y0 = -(-self.padding_x // 2), -(-self.padding_y // 2)
        x1, y1 = -(-(self.padding_x + self.orig_width) // 2), -(-(self.padding_y + self.orig_height) // 2)
        return (x0, y0, x1 - x0, y1 - y0)

    def _stats_window(self, window):
        """The window of the statistics calls on cells: default_cell_window() by default, "all" for every cell."""
        if window is None:
            window = self.default_cell_window()
        return None if window == "all" else _window(window)

    def _frame_count(self):
        """Frames the context holds: the slots of an MFChain, else two per pair."""
        n = C.c_int()
        _capi.check(self._lib.bbme_chain_frames(self._ctx, C.byref(n)))
        return n.value or 2 * getattr(self, "batch", 1)

    def _consistency_stats(self, which, tol, window):
        win = self._stats_window(window)
        pairs = getattr(self, "batch", 1)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_consistency_stats(self._ctx, _which(which), int(tol), win, s))
        return [dict(zip(("consistent", "inconsistent", "outside", "discrepancy"), s[4 * p:4 * p + 4])) for p in range(pairs)]

    def consistency_stats(self, which="forward", tol=1, window=None):
        """dict(consistent, inconsistent, outside, discrepancy) of that mask over window (cx0, cy0, cw, ch) in cells:
        cells per class and the sum of the discrepancy |dx + ex| + |dy + ey| over the cells of the first two.  Default
        window: default_cell_window(); "all": every cell of the padded grid."""
        return self._consistency_stats(which, tol, window)[0]

    def cells_consistency_device(self, a, b, tol=1, mask=None, stats=None, window=None, hip_stream_handle=None):
        """The consistency rule on any two cell grids in HBM: a, b contiguous int16 CUDA tensors (CH, CW, 2); mask a uint8
        CUDA tensor (CH, CW) whose rows may be further apart than CW (a column slice of a wider tensor); stats an int64 or
        uint64 CUDA tensor of 4 (consistent, inconsistent, outside, discrepancy) over window (cx0, cy0, cw, ch) in cells
        (None = all cells).  On the given HIP stream (default: the context's), ordered behind the context's stream; no host
        wait.  Needs no estimate."""
        import torch
        ch, cw = self.cells_shape
        for t in (a, b):
            if not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_consistency_device: grids must be contiguous int16 CUDA tensors "
                                      "of shape (%d, %d, 2)" % (ch, cw))
        if mask is not None and not (mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (ch, cw)
                                     and mask.stride(1) == 1 and mask.stride(0) >= cw):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_consistency_device: mask must be a uint8 CUDA tensor of shape "
                                  "(%d, %d) with unit column stride" % (ch, cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_consistency_device: stats must be a contiguous int64 or uint64 CUDA "
                                  "tensor of 4")
        win = _window(window)
        self._behind_torch(a, b, mask, stats)
        _capi.check(self._lib.bbme_cells_consistency_device(
            self._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), int(tol), win,
            C.c_void_p(mask.data_ptr() if mask is not None else 0), mask.stride(0) if mask is not None else 0,
            C.c_void_p(stats.data_ptr() if stats is not None else 0), C.c_void_p(hip_stream_handle or 0)))
        return mask, stats

    # -- quarter-pel refinement of the cells at the planes' own resolution (the SUBPEL RULE of include/bbme.h) -----------------------
    def _subpel_cells(self, pair, which, out, what):
        out = _host_out(out, self.cells_shape + (2,), np.int16, what)
        _capi.check(self._lib.bbme_get_subpel_cells_host(self._ctx, pair, _which(which), out.ctypes.data))
        return out

    def subpel_cells(self, which="forward", pair=0, out=None):
        """The context's cells refined to quarter-pel on its level-0 planes -> (CH, CW, 2) int16, 4 x integer vector + q with
        q in [-3, 3]^2.  which="forward": the current cells against (image 1, image 2), after estimate_async() or
        estimate_bidirectional_async(); "backward": the backward cells against (image 2, image 1).  An upsample=4 context
        refines its 4x planes (1/16 pel of the source)."""
        return self._subpel_cells(pair, which, out, "subpel_cells")

    def _subpel_flow(self, pair, which, out, what):
        out = _host_out(out, self.subsampled_shape(), np.float32, what)
        _capi.check(self._lib.bbme_get_subpel_flow_host(self._ctx, pair, _which(which), out.ctypes.data))
        return out

    def subpel_flow(self, which="forward", pair=0, out=None):
        """The refined field of the unpadded source frame -> (H, W, 2) float32 in pixels of the source: every pixel its cell's
        quarter-pel vector / 4; on an upsample=4 context every 4th pixel of the 4x frame, / 16.  Ready for Flow.write_flow_file
        and Flow.calculate_mse."""
        return self._subpel_flow(pair, which, out, "subpel_flow")

    def _subpel_stats(self, which, window):
        win = self._stats_window(window)
        pairs = getattr(self, "batch", 1)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_subpel_stats(self._ctx, _which(which), win, s))
        return [dict(zip(_SUBPEL_STATS, s[4 * p:4 * p + 4])) for p in range(pairs)]

    def subpel_stats(self, which="forward", window=None):
        """dict(valid, moved, cost_integer, cost_refined) of the refinement over window (cx0, cy0, cw, ch) in cells: valid cells,
        cells with q != (0, 0), and the sums of the 8x8 window's SAD at the integer vector and at the refined one over the
        valid cells.  Default window: default_cell_window(); "all": every cell of the padded grid."""
        return self._subpel_stats(which, window)[0]

    def cells_subpel_device(self, i1, i2, cells, out=None, stats=None, window=None, stream=None):
        """The subpel rule on any two planes and any cell grid in HBM: i1, i2 contiguous uint8 CUDA tensors (H_pad, W_pad), cells a
        contiguous int16 CUDA tensor (CH, CW, 2); out an int16 CUDA tensor (CH, CW, 2) whose rows may be further apart than CW
        cells; stats an int64 or uint64 CUDA tensor of 4 (valid, moved, cost_integer, cost_refined) over window (cx0, cy0, cw, ch)
        in cells (None = all cells).  On the given HIP stream handle (default: the context's), ordered behind the context's
        stream; no host wait.  Needs no frames and no estimate."""
        import torch
        what = "cells_subpel_device"
        ch, cw = self.cells_shape
        for t in (i1, i2):
            if not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (2 * ch, 2 * cw) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: planes must be contiguous uint8 CUDA tensors of shape (%d, %d)"
                                      % (what, 2 * ch, 2 * cw))
        if not (cells.is_cuda and cells.dtype == torch.int16 and tuple(cells.shape) == (ch, cw, 2) and cells.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: cells must be a contiguous int16 CUDA tensor of shape (%d, %d, 2)"
                                  % (what, ch, cw))
        if out is not None and not (out.is_cuda and out.dtype == torch.int16 and tuple(out.shape) == (ch, cw, 2)
                                    and out.stride(2) == 1 and out.stride(1) == 2 and out.stride(0) >= 2 * cw
                                    and out.stride(0) % 2 == 0 and out.data_ptr() % 4 == 0):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be an int16 CUDA tensor of shape (%d, %d, 2) with packed cells "
                                  "and rows a whole number of cells apart" % (what, ch, cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 4" % what)
        win = _window(window)
        self._behind_torch(i1, i2, cells, out, stats)
        _capi.check(self._lib.bbme_cells_subpel_device(
            self._ctx, C.c_void_p(i1.data_ptr()), C.c_void_p(i2.data_ptr()), C.c_void_p(cells.data_ptr()), win,
            C.c_void_p(out.data_ptr() if out is not None else 0), out.stride(0) // 2 if out is not None else 0,
            C.c_void_p(stats.data_ptr() if stats is not None else 0), C.c_void_p(stream or 0)))
        return out, stats

    # -- motion compensation along the quarter-pel cells (the SUBPEL COMPENSATION RULE of include/bbme.h) ---------------------------
    def _get_subpel_compensated(self, pair, which, fill, out, what):
        out = _host_out(out, (self.padded_height, self.padded_width), np.uint8, what)
        _capi.check(self._lib.bbme_get_subpel_compensated_host(self._ctx, pair, _which(which), fill, out.ctypes.data))
        return out

    def draw_MVimage_subpel(self, which="forward", fill=0, out=None):
        """draw_MVimage(0, 2) along the cells refined to quarter-pel (subpel_cells(which)): the padded (H_pad, W_pad) uint8 plane,
        every 2x2 cell the bilinear quarter-pel samples of the other image where its vector points, cells whose samples leave
        the plane set to `fill`.  which="forward": image 1 predicted from image 2; "backward": image 2 from image 1 along the
        backward cells, after estimate_bidirectional_async().  An upsample=4 context compensates its 4x planes."""
        return self._get_subpel_compensated(0, which, fill, out, "draw_MVimage_subpel")

    def _subpel_compensation_stats(self, which, window):
        if window is None:
            window = (self.padding_x, self.padding_y, self.orig_width, self.orig_height)
        pairs = getattr(self, "batch", 1)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_subpel_compensation_error(self._ctx, _which(which), _window(window), s))
        return [_residual_dict(s[4 * p:4 * p + 4]) for p in range(pairs)]

    def compensation_error_subpel(self, which="forward", window=None):
        """Residual statistics of draw_MVimage_subpel(which) against the image it predicts (image 1 for "forward", image 2 for
        "backward") over window (x0, y0, w, h) in pixels of the padded plane: the dict of compensation_error.  Default window:
        the unpadded frame."""
        return self._subpel_compensation_stats(which, window)[0]

    def cells_compensate_subpel_device(self, i1, i2, q4, out=None, stats=None, fill=0, window=None, stream=None):
        """The subpel compensation rule on any planes and any quarter-pel grid in HBM: i1 (None without stats), i2 contiguous
        uint8 CUDA tensors (H_pad, W_pad); q4 an int16 CUDA tensor (CH, CW, 2) whose rows may be further apart than CW cells
        (what cells_subpel_device wrote); out a uint8 CUDA tensor (H_pad, W_pad) with unit column stride whose rows may be
        further apart than W_pad, at any byte address; stats an int64 or uint64 CUDA tensor of 4 (sse, sad, pixels, skipped)
        over window (x0, y0, w, h) in pixels (None = the whole plane).  On the given HIP stream handle (default: the
        context's), ordered behind the context's stream; no host wait.  Needs no frames and no estimate."""
        import torch
        what = "cells_compensate_subpel_device"
        ch, cw = self.cells_shape
        for t in (i2,) if i1 is None and stats is None else (i1, i2):
            if t is None or not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (2 * ch, 2 * cw) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: planes must be contiguous uint8 CUDA tensors of shape (%d, %d)"
                                      % (what, 2 * ch, 2 * cw))
        if not (q4.is_cuda and q4.dtype == torch.int16 and tuple(q4.shape) == (ch, cw, 2) and q4.stride(2) == 1
                and q4.stride(1) == 2 and q4.stride(0) >= 2 * cw and q4.stride(0) % 2 == 0 and q4.data_ptr() % 4 == 0):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: q4 must be an int16 CUDA tensor of shape (%d, %d, 2) with packed cells "
                                  "and rows a whole number of cells apart" % (what, ch, cw))
        if out is None and stats is None:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: neither out nor stats" % what)
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (2 * ch, 2 * cw)
                                    and out.stride(1) == 1 and out.stride(0) >= 2 * cw):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d) with unit column stride"
                                  % (what, 2 * ch, 2 * cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 4" % what)
        self._behind_torch(i1, i2, q4, out, stats)
        _capi.check(self._lib.bbme_cells_subpel_compensate_device(
            self._ctx, _ptr(i1), _ptr(i2), _ptr(q4), q4.stride(0) // 2, int(fill), _window(window), _ptr(out),
            out.stride(0) if out is not None else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, stats

    # -- global motion and global compensation (the GLOBAL MOTION RULE and the GLOBAL COMPENSATION RULE of include/bbme.h) ----------
    def _global_motion(self, which, subpel, kind, tol, iterations, mask_tol, window):
        """Every pair's estimate from one launch per step -> list of dicts without the map."""
        pairs = getattr(self, "batch", 1)
        unit = 4 if subpel else 1
        models = np.zeros((pairs, 6), np.int32)
        words = np.zeros((pairs, 16), np.int64)
        _capi.check(self._lib.bbme_global_motion(self._ctx, _which(which), int(bool(subpel)), _gm_kind(kind), _gm_tol(tol, unit),
                                                 int(iterations), -1 if mask_tol is None else int(mask_tol), self._stats_window(window),
                                                 models.ctypes.data, words.ctypes.data))
        return [_gm_dict(models[p], words[p], unit) for p in range(pairs)]

    def _global_motion_map(self, pair, which, subpel, mask_tol, model, tol, out, what):
        out = _host_out(out, self.cells_shape, np.uint8, what)
        model = _gm_model(model, what)
        _capi.check(self._lib.bbme_get_global_motion_map_host(self._ctx, pair, _which(which), int(bool(subpel)),
                                                              -1 if mask_tol is None else int(mask_tol), model.ctypes.data,
                                                              _gm_tol(tol, 4 if subpel else 1), out.ctypes.data))
        return out

    def global_motion(self, which="forward", subpel=False, kind="affine", tol=1.0, iterations=3, mask_tol=None, window=None):
        """The dominant motion of the context's cells (the global motion rule): dict(model, unit, translation, statistics, map).
        model: six int32 in Q16 (m0..m2 for u, m3..m5 for v) in grid units of 1 / unit pixel over half pixels from the plane
        centre; translation: (m0, m3) in pixels; statistics: dict(inliers, outliers, excluded, residual, ...) of the last
        moments pass; map: (CH, CW) uint8, 0 a cell that follows the model within `tol` pixels (L1), 1 one that does not, 2 an
        excluded one.  which: the forward (current) or the backward cells; subpel: refine them to quarter-pel first (unit 4);
        kind: "translation" or "affine"; mask_tol: exclude the cells that consistency(which, mask_tol) does not call consistent
        (needs estimate_bidirectional_async()); window (cx0, cy0, cw, ch) in cells, default default_cell_window(), "all" every
        cell.  Synchronises at every step."""
        d = self._global_motion(which, subpel, kind, tol, iterations, mask_tol, window)[0]
        d["map"] = self._global_motion_map(0, which, subpel, mask_tol, d["model"], tol, None, "global_motion")
        return d

    def _get_global_compensated(self, pair, which, model, unit, fill, out, what):
        out = _host_out(out, (self.padded_height, self.padded_width), np.uint8, what)
        model = _gm_model(model, what)
        _capi.check(self._lib.bbme_get_global_compensated_host(self._ctx, pair, _which(which), model.ctypes.data, int(unit), int(fill),
                                                               out.ctypes.data))
        return out

    def draw_MVimage_global(self, model, unit=1, which="forward", fill=0, out=None):
        """The padded (H_pad, W_pad) uint8 plane compensated for the model's motion alone (the global compensation rule): every
        pixel the bilinear quarter-pel sample of the other image where the model points, `fill` where a tap leaves the plane.
        which="forward": image 1 predicted from image 2; "backward": image 2 from image 1.  Needs frames, no estimate."""
        return self._get_global_compensated(0, which, model, unit, fill, out, "draw_MVimage_global")

    def _global_compensation_stats(self, which, models, unit, window):
        if window is None:
            window = (self.padding_x, self.padding_y, self.orig_width, self.orig_height)
        pairs = getattr(self, "batch", 1)
        models = np.ascontiguousarray(models, np.int32).reshape(-1)
        if models.size != 6 * pairs:
            raise _capi.BbmeError(_capi.ERR_INVALID, "compensation_error_global: six int32 per pair (%d pairs)" % pairs)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_global_compensation_error(self._ctx, _which(which), models.ctypes.data, int(unit), _window(window), s))
        return [_residual_dict(s[4 * p:4 * p + 4]) for p in range(pairs)]

    def compensation_error_global(self, model, unit=1, which="forward", window=None):
        """Residual statistics of draw_MVimage_global against the image it predicts over window (x0, y0, w, h) in pixels of the
        padded plane: the dict of compensation_error.  Default window: the unpadded frame."""
        return self._global_compensation_stats(which, model, unit, window)[0]

    def _check_gm_grid_tensors(self, cells, exclude, what):
        import torch
        ch, cw = self.cells_shape
        if not (cells.is_cuda and cells.dtype == torch.int16 and tuple(cells.shape) == (ch, cw, 2) and cells.stride(2) == 1
                and cells.stride(1) == 2 and cells.stride(0) >= 2 * cw and cells.stride(0) % 2 == 0 and cells.data_ptr() % 4 == 0):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: cells must be an int16 CUDA tensor of shape (%d, %d, 2) with packed cells "
                                  "and rows a whole number of cells apart" % (what, ch, cw))
        if exclude is not None and not (exclude.is_cuda and exclude.dtype == torch.uint8 and tuple(exclude.shape) == (ch, cw)
                                        and exclude.stride(1) == 1 and exclude.stride(0) >= cw):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: exclude must be a uint8 CUDA tensor of shape (%d, %d) with unit column "
                                  "stride" % (what, ch, cw))

    def cells_vector_histogram_device(self, cells, hist, exclude=None, window=None, stream=None):
        """The histogram part of the global motion rule on any grid in HBM: cells an int16 CUDA tensor (CH, CW, 2) whose rows may
        be further apart than CW cells, exclude a uint8 CUDA tensor (CH, CW) with unit column stride (non-zero = excluded) or
        None, hist a contiguous int32 or uint32 CUDA tensor of 2 x 2048 (zeroed and filled), window (cx0, cy0, cw, ch) in
        cells (None = all).  On the given HIP stream handle (default: the context's), ordered behind the context's stream; no
        host wait.  Needs no estimate."""
        import torch
        what = "cells_vector_histogram_device"
        self._check_gm_grid_tensors(cells, exclude, what)
        if not (hist.is_cuda and hist.dtype in (torch.int32, torch.uint32) and hist.numel() == 4096 and hist.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: hist must be a contiguous int32 or uint32 CUDA tensor of 4096" % what)
        self._behind_torch(cells, exclude, hist)
        _capi.check(self._lib.bbme_cells_vector_histogram_device(
            self._ctx, _ptr(cells), cells.stride(0) // 2, _ptr(exclude), exclude.stride(0) if exclude is not None else 0,
            _window(window), _ptr(hist), C.c_void_p(stream or 0)))
        return hist

    def cells_global_moments_device(self, cells, model, tol_q16, exclude=None, map=None, words=None, window=None, stream=None):
        """The moments part of the global motion rule on any grid in HBM: cells and exclude as for
        cells_vector_histogram_device, model six int32 (host), tol_q16 the tolerance in Q16 grid units; map a uint8 CUDA tensor
        (CH, CW) with unit column stride whose rows may be further apart than CW; words a contiguous int64 CUDA tensor of 16.
        Same stream rules; no host wait."""
        import torch
        what = "cells_global_moments_device"
        ch, cw = self.cells_shape
        self._check_gm_grid_tensors(cells, exclude, what)
        if map is None and words is None:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: neither map nor words" % what)
        if map is not None and not (map.is_cuda and map.dtype == torch.uint8 and tuple(map.shape) == (ch, cw) and map.stride(1) == 1
                                    and map.stride(0) >= cw):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: map must be a uint8 CUDA tensor of shape (%d, %d) with unit column stride"
                                  % (what, ch, cw))
        if words is not None and not (words.is_cuda and words.dtype in (torch.int64, torch.uint64) and words.numel() == 16
                                      and words.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: words must be a contiguous int64 CUDA tensor of 16" % what)
        model = _gm_model(model, what)
        self._behind_torch(cells, exclude, map, words)
        _capi.check(self._lib.bbme_cells_global_moments_device(
            self._ctx, _ptr(cells), cells.stride(0) // 2, _ptr(exclude), exclude.stride(0) if exclude is not None else 0,
            model.ctypes.data, int(tol_q16), _window(window), _ptr(map), map.stride(0) if map is not None else 0, _ptr(words),
            C.c_void_p(stream or 0)))
        return map, words

    def cells_global_compensate_device(self, i1, i2, model, unit=1, out=None, stats=None, fill=0, window=None, stream=None):
        """The global compensation rule on any planes in HBM: i1 (None without stats), i2 contiguous uint8 CUDA tensors
        (H_pad, W_pad); model six int32 (host) in grid units of 1 / unit pixel; out a uint8 CUDA tensor (H_pad, W_pad) with unit
        column stride whose rows may be further apart than W_pad; stats an int64 or uint64 CUDA tensor of 4 (sse, sad, pixels,
        skipped) over window (x0, y0, w, h) in pixels (None = the whole plane).  Same stream rules; no host wait.  Needs no
        frames and no estimate."""
        import torch
        what = "cells_global_compensate_device"
        ch, cw = self.cells_shape
        for t in (i2,) if i1 is None and stats is None else (i1, i2):
            if t is None or not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (2 * ch, 2 * cw) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: planes must be contiguous uint8 CUDA tensors of shape (%d, %d)"
                                      % (what, 2 * ch, 2 * cw))
        if out is None and stats is None:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: neither out nor stats" % what)
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (2 * ch, 2 * cw)
                                    and out.stride(1) == 1 and out.stride(0) >= 2 * cw):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d) with unit column stride"
                                  % (what, 2 * ch, 2 * cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 4" % what)
        model = _gm_model(model, what)
        self._behind_torch(i1, i2, out, stats)
        _capi.check(self._lib.bbme_cells_global_compensate_device(
            self._ctx, _ptr(i1), _ptr(i2), model.ctypes.data, int(unit), int(fill), _window(window), _ptr(out),
            out.stride(0) if out is not None else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, stats

    # -- the same on the B,G,R frames (the BGR GLOBAL COMPENSATION RULE of include/bbme.h): needs frames set as (H, W, 3) ---------
    def _get_global_compensated_bgr(self, pair, which, model, unit, fill, out, what):
        out = _host_out(out, (self.orig_height, self.orig_width, 3), np.uint8, what)
        model = _gm_model(model, what)
        _capi.check(self._lib.bbme_get_global_compensated_bgr_host(self._ctx, pair, _which(which), model.ctypes.data, int(unit),
                                                                   int(fill), out.ctypes.data))
        return out

    def draw_MVimage_global_bgr(self, model, unit=1, which="forward", fill=0, out=None):
        """draw_MVimage_global in colour: the UNPADDED (H, W, 3) uint8 frame compensated for the model's motion alone (the BGR
        global compensation rule), sampled from the stored B,G,R frame of the other image; a source in the padding reads its
        zero, one outside the padded plane gives `fill`.  BbmeError (ERR_STATE) when a frame of the pair was set grey."""
        return self._get_global_compensated_bgr(0, which, model, unit, fill, out, "draw_MVimage_global_bgr")

    def _global_compensation_stats_bgr(self, which, models, unit, window):
        pairs = getattr(self, "batch", 1)
        models = np.ascontiguousarray(models, np.int32).reshape(-1)
        if models.size != 6 * pairs:
            raise _capi.BbmeError(_capi.ERR_INVALID, "compensation_error_global_bgr: six int32 per pair (%d pairs)" % pairs)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_global_compensation_error_bgr(self._ctx, _which(which), models.ctypes.data, int(unit),
                                                                 _window(window), s))
        return [_residual_dict(s[4 * p:4 * p + 4], 3) for p in range(pairs)]

    def compensation_error_global_bgr(self, model, unit=1, which="forward", window=None):
        """Residual statistics of draw_MVimage_global_bgr against the colour frame it predicts over window (x0, y0, w, h) in
        pixels of the FRAME (None = the whole frame): the dict of compensation_error_global with sse and sad summed over the three
        channels and mse = sse / (3 pixels)."""
        return self._global_compensation_stats_bgr(which, model, unit, window)[0]

    def cells_global_compensate_bgr_device(self, bgr1, bgr2, models, unit=1, out=None, stats=None, fill=0, window=None, stream=None):
        """The BGR global compensation rule on any colour frames in HBM, a run of them from ONE launch: bgr1 (None without stats)
        and bgr2 uint8 CUDA tensors (H, W, 3) or (N, H, W, 3), N <= GC_MAX_FRAMES, with packed pixels, a common row pitch and a
        common frame stride; models (6,) or (N, 6) int32 on the host, frame k under models[k]; out a uint8 CUDA tensor of the same
        shape with packed pixels whose rows and frames may be further apart; stats an int64 or uint64 CUDA tensor of 4 N (sse,
        sad, pixels, skipped per frame) over window (x0, y0, w, h) in frame pixels (None = the whole frame).  On the given HIP
        stream handle (default: the context's), ordered behind the context's stream; no host wait.  Needs no frames and no
        estimate."""
        import torch
        what = "cells_global_compensate_bgr_device"
        h, w = self.orig_height, self.orig_width
        if bgr2 is None or bgr2.dim() not in (3, 4):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: bgr2 must be a uint8 CUDA tensor (H, W, 3) or (N, H, W, 3)" % what)
        run = bgr2.dim() == 4
        count = bgr2.shape[0] if run else 1
        shape = ((count,) if run else ()) + (h, w, 3)

        def frames_ok(t):
            return t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == shape and _packed_pixels(t[0] if run else t)

        for t in (bgr2,) if bgr1 is None and stats is None else (bgr1, bgr2):
            if t is None or not (frames_ok(t) and t.stride(-3) == bgr2.stride(-3) and (not run or t.stride(0) == bgr2.stride(0))):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: colour frames must be uint8 CUDA tensors of shape %s with packed pixels, "
                                      "a common row pitch and a common frame stride" % (what, shape))
        if out is None and stats is None:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: neither out nor stats" % what)
        if out is not None and not frames_ok(out):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape %s with packed pixels" % (what, shape))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4 * count
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of %d" % (what, 4 * count))
        models = np.ascontiguousarray(models, np.int32).reshape(-1)
        if models.size != 6 * count:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: six int32 per frame (%d frames)" % (what, count))
        self._behind_torch(bgr1, bgr2, out, stats)
        _capi.check(self._lib.bbme_cells_global_compensate_bgr_device(
            self._ctx, _ptr(bgr1), _ptr(bgr2), bgr2.stride(-3), bgr2.stride(0) if run else 0, count, models.ctypes.data, int(unit),
            int(fill), _window(window), _ptr(out), out.stride(-3) if out is not None else 0,
            out.stride(0) if out is not None and run else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, stats

    # -- motion compensation of the B,G,R frames along the cells (the BGR COMPENSATION RULE of include/bbme.h): needs frames set as
    # (H, W, 3); unit 1 = the integer cells, unit 4 = the cells refined to quarter pels on the luma planes ------------------------
    def _get_compensated_bgr(self, pair, which, unit, fill, out, what):
        out = _host_out(out, (self.orig_height, self.orig_width, 3), np.uint8, what)
        _capi.check(self._lib.bbme_get_compensated_bgr_host(self._ctx, pair, _which(which), int(unit), int(fill), out.ctypes.data))
        return out

    def draw_MVimage_bgr(self, which="forward", fill=0, out=None):
        """draw_MVimage(0, 2) in colour: the UNPADDED (H, W, 3) uint8 frame, every 2x2 cell of the padded plane copied from the
        stored B,G,R frame of the other image where its integer vector points (the BGR compensation rule, unit 1); a source in
        the padding reads its zero, a cell whose source leaves the padded plane gives `fill`.  which="forward": frame 1 predicted
        from frame 2; "backward": frame 2 from frame 1 along the backward cells, after estimate_bidirectional_async().
        BbmeError (ERR_STATE) when a frame of the pair was set grey."""
        return self._get_compensated_bgr(0, which, 1, fill, out, "draw_MVimage_bgr")

    def draw_MVimage_subpel_bgr(self, which="forward", fill=0, out=None):
        """draw_MVimage_subpel in colour: as draw_MVimage_bgr along the cells refined to quarter pels on the luma planes
        (subpel_cells(which)), every channel sampled bilinearly (the BGR compensation rule, unit 4)."""
        return self._get_compensated_bgr(0, which, 4, fill, out, "draw_MVimage_subpel_bgr")

    def _compensation_stats_bgr(self, which, unit, window):
        pairs = getattr(self, "batch", 1)
        s = (C.c_ulonglong * (4 * pairs))()
        _capi.check(self._lib.bbme_compensation_error_bgr(self._ctx, _which(which), int(unit), _window(window), s))
        return [_residual_dict(s[4 * p:4 * p + 4], 3) for p in range(pairs)]

    def compensation_error_bgr(self, which="forward", window=None):
        """Residual statistics of draw_MVimage_bgr(which) against the colour frame it predicts over window (x0, y0, w, h) in
        pixels of the FRAME (None = the whole frame): the dict of compensation_error_global_bgr, sse and sad summed over the
        three channels and mse = sse / (3 pixels)."""
        return self._compensation_stats_bgr(which, 1, window)[0]

    def compensation_error_subpel_bgr(self, which="forward", window=None):
        """The same of draw_MVimage_subpel_bgr(which)."""
        return self._compensation_stats_bgr(which, 4, window)[0]

    def cells_compensate_bgr_device(self, bgr1, bgr2, grid, unit, out=None, stats=None, fill=0, window=None, stream=None):
        """The BGR compensation rule on any colour frames and any grid in HBM: bgr1 (None without stats) and bgr2 uint8 CUDA
        tensors (H, W, 3) with packed pixels and a common row pitch; grid an int16 CUDA tensor (CH, CW, 2) whose rows may be
        further apart than CW cells, integer cells with unit=1 or quarter-pel vectors with unit=4 (what cells_subpel_device
        wrote); out a uint8 CUDA tensor (H, W, 3) with packed pixels whose rows may be further apart, at any byte address; stats
        an int64 or uint64 CUDA tensor of 4 (sse, sad, pixels, skipped) over window (x0, y0, w, h) in frame pixels (None = the
        whole frame).  On the given HIP stream handle (default: the context's), ordered behind the context's stream; no host
        wait.  Needs no frames and no estimate."""
        import torch
        what = "cells_compensate_bgr_device"
        shape = (self.orig_height, self.orig_width, 3)
        ch, cw = self.cells_shape

        def frame_ok(t):
            return t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == shape and _packed_pixels(t)

        for t in (bgr2,) if bgr1 is None and stats is None else (bgr1, bgr2):
            if t is None or not (frame_ok(t) and t.stride(0) == bgr2.stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: colour frames must be uint8 CUDA tensors of shape %s with packed pixels "
                                      "and a common row pitch" % (what, shape))
        if not (grid.is_cuda and grid.dtype == torch.int16 and tuple(grid.shape) == (ch, cw, 2) and grid.stride(2) == 1
                and grid.stride(1) == 2 and grid.stride(0) >= 2 * cw and grid.stride(0) % 2 == 0 and grid.data_ptr() % 4 == 0):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: grid must be an int16 CUDA tensor of shape (%d, %d, 2) with packed cells "
                                  "and rows a whole number of cells apart" % (what, ch, cw))
        if out is None and stats is None:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: neither out nor stats" % what)
        if out is not None and not frame_ok(out):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape %s with packed pixels" % (what, shape))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 4" % what)
        self._behind_torch(bgr1, bgr2, grid, out, stats)
        _capi.check(self._lib.bbme_cells_compensate_bgr_device(
            self._ctx, _ptr(bgr1), _ptr(bgr2), bgr2.stride(0), _ptr(grid), grid.stride(0) // 2, int(unit), int(fill), _window(window),
            _ptr(out), out.stride(0) if out is not None else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, stats

    # -- colour coding of the field: Flow::MotionToColor on the GPU, from the cells (the colour rule of include/bbme.h) ----------
    def color_shape(self, scale=None):
        """(rows, cols, 3) of the colour image: the subsampled field's size; scale defaults to upsample."""
        return self.subsampled_shape(scale)[:2] + (3,)

    def _get_flow_color(self, pair, scale, maxmotion, which, out, what):
        shape = self.color_shape(scale)
        scale = self.upsample if scale is None else int(scale)
        out = _host_out(out, shape, np.uint8, what)
        rng = (C.c_float * 5)()
        _capi.check(self._lib.bbme_get_flow_color_host(self._ctx, pair, _which(which), scale, float(maxmotion), out.ctypes.data, rng))
        self.last_color_range = tuple(rng)
        return out

    def flow_color(self, scale=None, maxmotion=-1.0, which="forward", pair=0, out=None):
        """Flow::MotionToColor of get_subsampled_flow(scale) without the field ever leaving the GPU -> (rows, cols, 3) uint8,
        B,G,R; only the image is downloaded.  which="backward": the backward field after estimate_bidirectional_async().
        maxmotion > 0 replaces the normalising radius.  Sets last_color_range = (max radius, min u, max u, min v, max v).
        The hue angle is the double atan2 rounded to float (include/bbme.h), so a channel may be one level from
        Flow().MotionToColor's where the platform's float atan2 rounds the other way."""
        return self._get_flow_color(pair, scale, maxmotion, which, out, "flow_color")

    def _color_tensors(self, scale, out, range, what):
        import torch
        rows, cols, _ = self.color_shape(scale)
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (rows, cols, 3)
                                    and out.stride(2) == 1 and out.stride(1) == 3 and out.stride(0) >= 3 * cols):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d, 3) with packed "
                                  "pixels" % (what, rows, cols))
        if range is not None and not (range.is_cuda and range.dtype == torch.float32 and range.numel() == 5 and range.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: range must be a contiguous float32 CUDA tensor of 5" % what)
        return (C.c_void_p(out.data_ptr() if out is not None else 0), out.stride(0) if out is not None else 0,
                C.c_void_p(range.data_ptr() if range is not None else 0))

    def flow_color_device(self, out, scale=None, maxmotion=-1.0, which="forward", pair=0, range=None, hip_stream_handle=None):
        """flow_color into a uint8 CUDA tensor of shape (rows, cols, 3) whose rows may be further apart than 3 cols bytes (a
        column slice of a wider tensor; any alignment), and / or the five range floats into a float32 CUDA tensor; on the
        given HIP stream (default: the context's), ordered behind the context's stream; no host wait."""
        scale = self.upsample if scale is None else int(scale)
        o, pitch, r = self._color_tensors(scale, out, range, "flow_color_device")
        self._behind_torch(out, range)
        _capi.check(self._lib.bbme_flow_color_device(self._ctx, pair, _which(which), scale, float(maxmotion), o, pitch, r,
                                                     C.c_void_p(hip_stream_handle or 0)))
        return out, range

    def cells_color_device(self, cells, out=None, range=None, scale=None, maxmotion=-1.0, hip_stream_handle=None):
        """The colour rule on any cell grid in HBM: cells a contiguous int16 CUDA tensor (CH, CW, 2); out and range as in
        flow_color_device, each may be None.  Needs no estimate."""
        import torch
        ch, cw = self.cells_shape
        if not (cells.is_cuda and cells.dtype == torch.int16 and tuple(cells.shape) == (ch, cw, 2) and cells.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_color_device: cells must be a contiguous int16 CUDA tensor of shape "
                                  "(%d, %d, 2)" % (ch, cw))
        scale = self.upsample if scale is None else int(scale)
        o, pitch, r = self._color_tensors(scale, out, range, "cells_color_device")
        self._behind_torch(cells, out, range)
        _capi.check(self._lib.bbme_cells_color_device(self._ctx, C.c_void_p(cells.data_ptr()), scale, float(maxmotion), o, pitch, r,
                                                      C.c_void_p(hip_stream_handle or 0)))
        return out, range

    def _flow_ranges(self, which, scale):
        scale = self.upsample if scale is None else int(scale)
        out = np.empty((getattr(self, "batch", 1), 5), np.float32)
        _capi.check(self._lib.bbme_flow_ranges(self._ctx, _which(which), scale, out.ctypes.data))
        return out

    def flow_range(self, which="forward", scale=None):
        """(max radius, min u, max u, min v, max v) of the subsampled field, from the cells on the GPU."""
        return tuple(float(v) for v in self._flow_ranges(which, scale)[0])

    # -- motion-compensated interpolation between the two frames (the interpolation rule of include/bbme.h) ---------------
    def _out_shape(self, bgr):
        """What interpolation and the temporal filter write: the padded grey plane or, in colour, the unpadded B,G,R frame."""
        return (self.orig_height, self.orig_width, 3) if bgr else (self.padded_height, self.padded_width)

    def _get_interpolated(self, pair, num, den, out, what, bgr=False, subpel=False):
        out = _host_out(out, self._out_shape(bgr), np.uint8, what)
        get = ((self._lib.bbme_get_subpel_interpolated_bgr_host if subpel else self._lib.bbme_get_interpolated_bgr_host) if bgr
               else self._lib.bbme_get_subpel_interpolated_host if subpel else self._lib.bbme_get_interpolated_host)
        _capi.check(get(self._ctx, pair, int(num), int(den), out.ctypes.data))
        return out

    def _interpolate_run(self, den, pair, what, bgr, subpel=False):
        import torch
        den = int(den)
        if not 2 <= den <= 256:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s %d outside 2..256" % (what, den))
        frames = torch.empty((den - 1,) + self._out_shape(bgr), dtype=torch.uint8, device="cuda:%d" % self.device)
        run = ((self._lib.bbme_subpel_interpolate_bgr_device if subpel else self._lib.bbme_interpolate_bgr_device) if bgr
               else self._lib.bbme_subpel_interpolate_device if subpel else self._lib.bbme_interpolate_device)
        _capi.check(run(self._ctx, pair, 1, den - 1, den, _ptr(frames), frames.stride(1), frames.stride(0), None))
        self.synchronize()
        return frames.cpu().numpy()

    def interpolate(self, num=1, den=2, pair=0, out=None):
        """The frame at phase num / den between image1 (phase 0) and image2 (phase 1) after estimate_bidirectional_async():
        every 2x2 cell motion-compensated along the forward vector, the reversed backward vector or no motion, whichever
        matches best, and blended -> the padded (H_pad, W_pad) uint8 plane.  An upsample=4 context interpolates its 4x planes."""
        return self._get_interpolated(pair, num, den, out, "interpolate")

    def interpolate_run(self, den, pair=0):
        """All den - 1 phases 1 / den .. (den - 1) / den from one launch -> (den - 1, H_pad, W_pad) uint8."""
        return self._interpolate_run(den, pair, "interpolate_run: den", False)

    # -- colour frames out (the BGR interpolation rule of include/bbme.h): needs frames set as (H, W, 3) ------------------------
    def interpolate_bgr(self, num=1, den=2, pair=0, out=None):
        """interpolate() in colour: the selection of the grey frame, made on the luma planes, applied to the B,G,R frames the
        context was fed -> the UNPADDED (H, W, 3) uint8 frame.  BbmeError (ERR_STATE) when a frame of the pair was set grey."""
        return self._get_interpolated(pair, num, den, out, "interpolate_bgr", bgr=True)

    def interpolate_run_bgr(self, factor, pair=0):
        """All factor - 1 phases 1 / factor .. (factor - 1) / factor from one launch -> (factor - 1, H, W, 3) uint8."""
        return self._interpolate_run(factor, pair, "interpolate_run_bgr: factor", True)

    def cells_interpolate_bgr_device(self, fwd, bwd=None, bgr1=None, bgr2=None, num0=1, count=1, den=2, pair=0, out=None,
                                     hip_stream_handle=None):
        """The BGR interpolation rule on the context's luma planes of `pair` and any two cell grids in HBM (as
        cells_interpolate_device): bgr1, bgr2 uint8 CUDA tensors (H, W, 3) with packed pixels and a common row pitch, or both
        None for the colour the context stored; phases num0 .. num0 + count - 1 of den in one launch into out, a uint8 CUDA
        tensor (count, H, W, 3) with packed pixels whose rows and frames may be further apart than packed (any alignment).  On
        the given HIP stream (default: the context's), ordered behind the context's stream; no host wait.  Needs no estimate."""
        import torch
        ch, cw = self.cells_shape
        h, w = self.orig_height, self.orig_width
        count = int(count)
        for t in (fwd, bwd):
            if t is not None and not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_interpolate_bgr_device: grids must be contiguous int16 CUDA tensors "
                                      "of shape (%d, %d, 2)" % (ch, cw))
        for t in (bgr1, bgr2):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3) and _packed_pixels(t)
                                      and (bgr1 is None or t.stride(0) == bgr1.stride(0))):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_interpolate_bgr_device: colour frames must be uint8 CUDA tensors of "
                                      "shape (%d, %d, 3) with packed pixels and a common row pitch" % (h, w))
        if out is None or not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (count, h, w, 3)
                               and out.stride(3) == 1 and out.stride(2) == 3):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_interpolate_bgr_device: out must be a uint8 CUDA tensor of shape "
                                  "(%d, %d, %d, 3) with packed pixels" % (count, h, w))

        self._behind_torch(fwd, bwd, bgr1, bgr2, out)
        _capi.check(self._lib.bbme_cells_interpolate_bgr_device(
            self._ctx, pair, _ptr(fwd), _ptr(bwd), _ptr(bgr1), _ptr(bgr2), bgr1.stride(0) if bgr1 is not None else 0, int(num0), count,
            int(den), _ptr(out), out.stride(1), max(out.stride(0), 0), C.c_void_p(hip_stream_handle or 0)))
        return out

    def bgr_frames_device_ptrs(self, pair=0):
        """Device pointers of the two stored colour frames of `pair` (packed, pitch 3 W), bbme_bgr_frames_device_pair."""
        a, b = C.c_void_p(), C.c_void_p()
        _capi.check(self._lib.bbme_bgr_frames_device_pair(self._ctx, pair, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _interpolation_stats(self, num, den, window, subpel=False):
        win = self._stats_window(window)
        pairs = getattr(self, "batch", 1)
        s = (C.c_ulonglong * (4 * pairs))()
        stats = self._lib.bbme_subpel_interpolation_stats if subpel else self._lib.bbme_interpolation_stats
        _capi.check(stats(self._ctx, int(num), int(den), win, s))
        return [dict(zip(INTERPOLATION_STAT_KEYS, s[4 * p:4 * p + 4])) for p in range(pairs)]

    def interpolation_stats(self, num=1, den=2, window=None):
        """dict(forward, backward, zero, cost) of that frame over window (cx0, cy0, cw, ch) in cells: cells per selected
        hypothesis and the sum of the selected 2x2 SADs.  Default window: default_cell_window(); "all": every cell."""
        return self._interpolation_stats(num, den, window)[0]

    def cells_interpolate_device(self, fwd, bwd=None, num0=1, count=1, den=2, pair=0, out=None, sel=None, stats=None, window=None,
                                 hip_stream_handle=None):
        """The interpolation rule on the context's planes of `pair` and any two cell grids in HBM: fwd, bwd (may be None)
        contiguous int16 CUDA tensors (CH, CW, 2); phases num0 .. num0 + count - 1 of den in one launch into out, a uint8 CUDA
        tensor (count, H_pad, W_pad), sel, uint8 (count, CH, CW) -- rows and frames of both may be further apart than packed --,
        and stats, a contiguous int64 or uint64 CUDA tensor (count, 4) of (forward, backward, zero, cost) over window (cx0, cy0,
        cw, ch) in cells (None = all cells); each of the three may be None.  On the given HIP stream (default: the
        context's), ordered behind the context's stream; no host wait.  Needs frames, but no estimate."""
        import torch
        ch, cw = self.cells_shape
        count = int(count)
        for t in (fwd, bwd):
            if t is not None and not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_interpolate_device: grids must be contiguous int16 CUDA tensors "
                                      "of shape (%d, %d, 2)" % (ch, cw))
        for t, shape, name in ((out, (count, self.padded_height, self.padded_width), "out"), (sel, (count, ch, cw), "sel")):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == shape and t.stride(2) == 1):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_interpolate_device: %s must be a uint8 CUDA tensor of shape %s "
                                      "with unit column stride" % (name, shape))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and tuple(stats.shape) == (count, 4)
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_interpolate_device: stats must be a contiguous int64 or uint64 CUDA "
                                  "tensor of shape (%d, 4)" % count)
        win = _window(window)

        self._behind_torch(fwd, bwd, out, sel, stats)
        _capi.check(self._lib.bbme_cells_interpolate_device(
            self._ctx, pair, _ptr(fwd), _ptr(bwd), int(num0), count, int(den), win,
            _ptr(out), out.stride(1) if out is not None else 0, max(out.stride(0), 0) if out is not None else 0,
            _ptr(sel), sel.stride(1) if sel is not None else 0, max(sel.stride(0), 0) if sel is not None else 0,
            _ptr(stats), C.c_void_p(hip_stream_handle or 0)))
        return out, sel, stats

    # -- interpolation at quarter-pel positions (the SUBPEL INTERPOLATION RULE of include/bbme.h) ------------------------------
    def interpolate_subpel(self, num=1, den=2, pair=0, out=None):
        """interpolate() at quarter-pel positions: both fields refined to quarter-pel (subpel_cells("forward") and
        ("backward")), every 2x2 cell placed at its quarter-pel position of the phase and sampled bilinearly from both frames
        -> the padded (H_pad, W_pad) uint8 plane.  A block that moves an odd number of pixels lands where it belongs at
        phase 1 / 2.  An upsample=4 context interpolates its 4x planes, a colour context its luma planes."""
        return self._get_interpolated(pair, num, den, out, "interpolate_subpel", subpel=True)

    def interpolate_run_subpel(self, den, pair=0):
        """All den - 1 phases of interpolate_subpel from two refinement launches and one interpolation launch ->
        (den - 1, H_pad, W_pad) uint8."""
        return self._interpolate_run(den, pair, "interpolate_run_subpel: den", False, subpel=True)

    def interpolation_stats_subpel(self, num=1, den=2, window=None):
        """interpolation_stats of interpolate_subpel's frame: dict(forward, backward, zero, cost), the costs on the rounded
        quarter-pel samples."""
        return self._interpolation_stats(num, den, window, subpel=True)[0]

    def cells_interpolate_subpel_device(self, qf, qb=None, num0=1, count=1, den=2, pair=0, out=None, sel=None, stats=None,
                                        window=None, stream=None):
        """The subpel interpolation rule on the context's planes of `pair` and any two quarter-pel grids in HBM: qf, qb (may be
        None) int16 CUDA tensors (CH, CW, 2) with packed cells whose rows may be further apart than CW cells (what
        cells_subpel_device wrote), both with the same row pitch; out, sel and stats as in cells_interpolate_device.  On the
        given HIP stream handle (default: the context's), ordered behind the context's stream; no host wait.  Needs frames,
        but no estimate."""
        import torch
        what = "cells_interpolate_subpel_device"
        ch, cw = self.cells_shape
        count = int(count)
        for t in (qf, qb):
            if t is qb and qb is None:
                continue
            if t is None or not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.stride(2) == 1
                                 and t.stride(1) == 2 and t.stride(0) >= 2 * cw and t.stride(0) % 2 == 0 and t.data_ptr() % 4 == 0
                                 and t.stride(0) == qf.stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: grids must be int16 CUDA tensors of shape (%d, %d, 2) with packed "
                                      "cells and rows a common whole number of cells apart" % (what, ch, cw))
        for t, shape, name in ((out, (count, self.padded_height, self.padded_width), "out"), (sel, (count, ch, cw), "sel")):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == shape and t.stride(2) == 1):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: %s must be a uint8 CUDA tensor of shape %s with unit column stride"
                                      % (what, name, shape))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and tuple(stats.shape) == (count, 4)
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of shape (%d, 4)"
                                  % (what, count))
        win = _window(window)
        self._behind_torch(qf, qb, out, sel, stats)
        _capi.check(self._lib.bbme_cells_subpel_interpolate_device(
            self._ctx, pair, _ptr(qf), _ptr(qb), qf.stride(0) // 2, int(num0), count, int(den), win,
            _ptr(out), out.stride(1) if out is not None else 0, max(out.stride(0), 0) if out is not None else 0,
            _ptr(sel), sel.stride(1) if sel is not None else 0, max(sel.stride(0), 0) if sel is not None else 0,
            _ptr(stats), C.c_void_p(stream or 0)))
        return out, sel, stats

    # -- colour frames at quarter-pel positions (the BGR SUBPEL INTERPOLATION RULE of include/bbme.h) --------------------------
    def interpolate_subpel_bgr(self, num=1, den=2, pair=0, out=None):
        """interpolate_subpel() in colour: its selection, made on the luma planes at quarter-pel positions, applied to the B,G,R
        frames the context was fed, every pixel sampled bilinearly at its quarter-pel position in both -> the UNPADDED (H, W, 3)
        uint8 frame.  BbmeError (ERR_STATE) when a frame of the pair was set grey."""
        return self._get_interpolated(pair, num, den, out, "interpolate_subpel_bgr", bgr=True, subpel=True)

    def interpolate_run_subpel_bgr(self, factor, pair=0):
        """All factor - 1 phases of interpolate_subpel_bgr from two refinement launches and one interpolation launch ->
        (factor - 1, H, W, 3) uint8."""
        return self._interpolate_run(factor, pair, "interpolate_run_subpel_bgr: factor", True, subpel=True)

    def cells_interpolate_subpel_bgr_device(self, qf, qb=None, bgr1=None, bgr2=None, num0=1, count=1, den=2, pair=0, out=None,
                                            stream=None):
        """The BGR subpel interpolation rule on the context's luma planes of `pair` and any two quarter-pel grids in HBM (as
        cells_interpolate_subpel_device: rows may be further apart than CW cells, both with the same row pitch): bgr1, bgr2
        uint8 CUDA tensors (H, W, 3) with packed pixels and a common row pitch, or both None for the colour the context stored;
        phases num0 .. num0 + count - 1 of den in one launch into out, a uint8 CUDA tensor (count, H, W, 3) with packed pixels
        whose rows and frames may be further apart than packed (any alignment).  On the given HIP stream handle (default: the
        context's), ordered behind the context's stream; no host wait.  Needs frames, but no estimate."""
        import torch
        what = "cells_interpolate_subpel_bgr_device"
        ch, cw = self.cells_shape
        h, w = self.orig_height, self.orig_width
        count = int(count)
        for t in (qf, qb):
            if t is qb and qb is None:
                continue
            if t is None or not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.stride(2) == 1
                                 and t.stride(1) == 2 and t.stride(0) >= 2 * cw and t.stride(0) % 2 == 0 and t.data_ptr() % 4 == 0
                                 and t.stride(0) == qf.stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: grids must be int16 CUDA tensors of shape (%d, %d, 2) with packed "
                                      "cells and rows a common whole number of cells apart" % (what, ch, cw))
        for t in (bgr1, bgr2):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3) and _packed_pixels(t)
                                      and (bgr1 is None or t.stride(0) == bgr1.stride(0))):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: colour frames must be uint8 CUDA tensors of shape (%d, %d, 3) with "
                                      "packed pixels and a common row pitch" % (what, h, w))
        if out is None or not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (count, h, w, 3)
                               and out.stride(3) == 1 and out.stride(2) == 3):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d, %d, 3) with packed "
                                  "pixels" % (what, count, h, w))
        self._behind_torch(qf, qb, bgr1, bgr2, out)
        _capi.check(self._lib.bbme_cells_subpel_interpolate_bgr_device(
            self._ctx, pair, _ptr(qf), _ptr(qb), qf.stride(0) // 2, _ptr(bgr1), _ptr(bgr2), bgr1.stride(0) if bgr1 is not None else 0,
            int(num0), count, int(den), _ptr(out), out.stride(1), max(out.stride(0), 0), C.c_void_p(stream or 0)))
        return out

    # -- motion-compensated temporal filter of a frame with its neighbours (the temporal filter rule of include/bbme.h) ------
    def _get_temporal_filtered(self, pair, which, strength, out, what, bgr=False, subpel=False):
        out = _host_out(out, self._out_shape(bgr), np.uint8, what)
        get = self._lib.bbme_get_temporal_filtered_bgr_host if bgr else self._lib.bbme_get_temporal_filtered_host
        if subpel:
            get = self._lib.bbme_get_subpel_temporal_filtered_bgr_host if bgr else self._lib.bbme_get_subpel_temporal_filtered_host
        _capi.check(get(self._ctx, pair, int(which), int(strength), out.ctypes.data))
        return out

    def _temporal_filter_stats(self, strength, window, bgr, subpel=False):
        frames = self._frame_count()
        s = (C.c_ulonglong * (4 * frames))()
        stats = self._lib.bbme_temporal_filter_bgr_stats if bgr else self._lib.bbme_temporal_filter_stats
        if subpel:
            stats = self._lib.bbme_subpel_temporal_filter_bgr_stats if bgr else self._lib.bbme_subpel_temporal_filter_stats
        _capi.check(stats(self._ctx, int(strength), self._stats_window(window), s))
        return [dict(zip(TEMPORAL_STAT_KEYS, s[4 * f:4 * f + 4])) for f in range(frames)]

    def temporal_filter(self, strength, which=0, pair=0, out=None):
        """Frame `which` (0 = image1, 1 = image2) of the pair after estimate_bidirectional_async(), averaged with its
        motion-aligned neighbour wherever their 2x2 cells match better than `strength` (1..1021, a 2x2 SAD) -> the padded
        (H_pad, W_pad) uint8 plane.  image1 is filtered with image2 along the forward cells, image2 with image1 along the
        backward cells; on an MFChain the frame is slot pair + which and uses both neighbours where it has them."""
        return self._get_temporal_filtered(pair, which, strength, out, "temporal_filter")

    def temporal_filter_stats(self, strength, window=None):
        """One dict(prev_cells, next_cells, weight, change) per frame of the context, from one launch, over window (cx0, cy0, cw,
        ch) in cells: cells that took their previous / next neighbour, the sum of the weights and the sum of |out - frame| over
        the window's pixels.  Frames in the order image1, image2 of pair 0, of pair 1, ...; on an MFChain slot by slot.  Default
        window: default_cell_window(); "all": every cell."""
        return self._temporal_filter_stats(strength, window, False)

    def cells_temporal_filter_device(self, cur, prev=None, next=None, to_prev=None, to_next=None, strength=64, out=None, weights=None,
                                     stats=None, window=None, hip_stream_handle=None):
        """The temporal filter rule on any three planes and any two cell grids in HBM: cur, prev, next contiguous uint8 CUDA
        tensors (H_pad, W_pad), to_prev, to_next contiguous int16 CUDA tensors (CH, CW, 2) on cur; a neighbour is its plane and
        its grid, either neighbour may be None.  Into out, a uint8 CUDA tensor (H_pad, W_pad), weights, uint8 (CH, CW) holding
        wP | wN << 4 -- rows of both may be further apart than packed --, and stats, a contiguous int64 or uint64 CUDA tensor of 4
        (TEMPORAL_STAT_KEYS) over window (cx0, cy0, cw, ch) in cells (None = all cells); each of the three may be None.  On the
        given HIP stream (default: the context's), ordered behind the context's stream; no host wait.  Needs neither frames nor
        an estimate."""
        import torch
        ch, cw = self.cells_shape
        h, w = self.padded_height, self.padded_width
        for t in (cur, prev, next):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_device: planes must be contiguous uint8 CUDA tensors "
                                      "of shape (%d, %d)" % (h, w))
        for t in (to_prev, to_next):
            if t is not None and not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_device: grids must be contiguous int16 CUDA tensors "
                                      "of shape (%d, %d, 2)" % (ch, cw))
        for t, shape, name in ((out, (h, w), "out"), (weights, (ch, cw), "weights")):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == shape and t.stride(1) == 1):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_device: %s must be a uint8 CUDA tensor of shape %s "
                                      "with unit column stride" % (name, shape))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_device: stats must be a contiguous int64 or uint64 CUDA "
                                  "tensor of 4")
        win = _window(window)

        self._behind_torch(cur, prev, next, to_prev, to_next, out, weights, stats)
        _capi.check(self._lib.bbme_cells_temporal_filter_device(
            self._ctx, _ptr(prev), _ptr(cur), _ptr(next), _ptr(to_prev), _ptr(to_next), int(strength), win,
            _ptr(out), out.stride(0) if out is not None else 0, _ptr(weights), weights.stride(0) if weights is not None else 0,
            _ptr(stats), C.c_void_p(hip_stream_handle or 0)))
        return out, weights, stats

    # -- the same along quarter-pel grids (the SUBPEL TEMPORAL FILTER RULE of include/bbme.h) ----------------------------------
    def temporal_filter_subpel(self, strength, which=0, pair=0, out=None):
        """temporal_filter() at quarter-pel positions: the integer cells the frame's neighbours hang on are refined
        (subpel_cells) and each neighbour's 2x2 cell is sampled bilinearly at its quarter-pel position; cost, weight and blend
        are temporal_filter()'s on the rounded samples -> the padded (H_pad, W_pad) uint8 plane."""
        return self._get_temporal_filtered(pair, which, strength, out, "temporal_filter_subpel", subpel=True)

    def temporal_filter_subpel_stats(self, strength, window=None):
        """temporal_filter_stats() of temporal_filter_subpel's frames: one dict(prev_cells, next_cells, weight, change) per frame
        of the context, from at most two refinement launches and one filter launch."""
        return self._temporal_filter_stats(strength, window, False, subpel=True)

    def cells_temporal_filter_subpel_device(self, cur, prev=None, next=None, q_to_prev=None, q_to_next=None, strength=64, out=None,
                                            weights=None, stats=None, window=None, stream=None):
        """The subpel temporal filter rule on any three planes and any two quarter-pel grids in HBM: planes, out, weights and
        stats as in cells_temporal_filter_device; q_to_prev, q_to_next int16 CUDA tensors (CH, CW, 2) on cur with packed cells
        whose rows may be further apart than CW cells (what cells_subpel_device wrote), both with the same row pitch.  On the
        given HIP stream handle (default: the context's), ordered behind the context's stream; no host wait.  Needs neither
        frames nor an estimate."""
        import torch
        what = "cells_temporal_filter_subpel_device"
        ch, cw = self.cells_shape
        h, w = self.padded_height, self.padded_width
        for t in (cur, prev, next):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: planes must be contiguous uint8 CUDA tensors of shape (%d, %d)"
                                      % (what, h, w))
        grids = [t for t in (q_to_prev, q_to_next) if t is not None]
        for t in grids:
            if not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.stride(2) == 1 and t.stride(1) == 2
                    and t.stride(0) >= 2 * cw and t.stride(0) % 2 == 0 and t.data_ptr() % 4 == 0 and t.stride(0) == grids[0].stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: grids must be int16 CUDA tensors of shape (%d, %d, 2) with packed "
                                      "cells and rows a common whole number of cells apart" % (what, ch, cw))
        for t, shape, name in ((out, (h, w), "out"), (weights, (ch, cw), "weights")):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == shape and t.stride(1) == 1):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: %s must be a uint8 CUDA tensor of shape %s with unit column stride"
                                      % (what, name, shape))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 4" % what)
        win = _window(window)
        self._behind_torch(cur, prev, next, q_to_prev, q_to_next, out, weights, stats)
        _capi.check(self._lib.bbme_cells_subpel_temporal_filter_device(
            self._ctx, _ptr(prev), _ptr(cur), _ptr(next), _ptr(q_to_prev), _ptr(q_to_next), grids[0].stride(0) // 2 if grids else cw,
            int(strength), win, _ptr(out), out.stride(0) if out is not None else 0, _ptr(weights),
            weights.stride(0) if weights is not None else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, weights, stats

    # -- the same on the B,G,R frames (the BGR temporal filter rule of include/bbme.h): needs frames set as (H, W, 3) -----------
    def temporal_filter_bgr(self, strength, which=0, pair=0, out=None):
        """temporal_filter() in colour: the stored B,G,R frame `which` averaged with its motion-aligned neighbour(s) wherever
        their 2x2 cells match better than `strength` in EVERY channel (the cost is the largest per-channel 2x2 SAD; the luma
        planes are not read) -> the UNPADDED (H, W, 3) uint8 frame.  Neighbours and grids as temporal_filter().  BbmeError
        (ERR_STATE) when the frame or a neighbour it uses was set grey."""
        return self._get_temporal_filtered(pair, which, strength, out, "temporal_filter_bgr", bgr=True)

    def temporal_filter_bgr_stats(self, strength, window=None):
        """temporal_filter_stats() of the colour filter: one dict(prev_cells, next_cells, weight, change) per frame of the context
        from one launch, over window (cx0, cy0, cw, ch) in cells of the padded view; `change` sums |out - frame| over the window's
        pixels and three channels.  Default window: default_cell_window(); "all": every cell."""
        return self._temporal_filter_stats(strength, window, True)

    def cells_temporal_filter_bgr_device(self, cur, prev=None, next=None, to_prev=None, to_next=None, strength=64, out=None,
                                         weights=None, stats=None, window=None, hip_stream_handle=None):
        """The BGR temporal filter rule on any three colour frames and any two cell grids in HBM: cur, prev, next uint8 CUDA
        tensors (H, W, 3) with packed pixels and a common row pitch, to_prev, to_next contiguous int16 CUDA tensors (CH, CW, 2) on
        cur; a neighbour is its frame and its grid, either neighbour may be None.  Into out, a uint8 CUDA tensor (H, W, 3) with
        packed pixels, weights, uint8 (CH, CW) holding wP | wN << 4 -- rows of both may be further apart than packed --, and
        stats, a contiguous int64 or uint64 CUDA tensor of 4 (TEMPORAL_STAT_KEYS) over window (cx0, cy0, cw, ch) in cells (None =
        all cells); each of the three may be None.  On the given HIP stream (default: the context's), ordered behind the
        context's stream; no host wait.  Needs neither frames nor an estimate."""
        import torch
        ch, cw = self.cells_shape
        h, w = self.orig_height, self.orig_width
        for t in (cur, prev, next):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3) and _packed_pixels(t)
                                      and cur is not None and t.stride(0) == cur.stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_bgr_device: colour frames must be uint8 CUDA tensors "
                                      "of shape (%d, %d, 3) with packed pixels and a common row pitch" % (h, w))
        for t in (to_prev, to_next):
            if t is not None and not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_bgr_device: grids must be contiguous int16 CUDA "
                                      "tensors of shape (%d, %d, 2)" % (ch, cw))
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and _packed_pixels(out)):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_bgr_device: out must be a uint8 CUDA tensor of shape "
                                  "(%d, %d, 3) with packed pixels" % (h, w))
        if weights is not None and not (weights.is_cuda and weights.dtype == torch.uint8 and tuple(weights.shape) == (ch, cw)
                                        and weights.stride(1) == 1):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_bgr_device: weights must be a uint8 CUDA tensor of shape "
                                  "(%d, %d) with unit column stride" % (ch, cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "cells_temporal_filter_bgr_device: stats must be a contiguous int64 or uint64 "
                                  "CUDA tensor of 4")
        win = _window(window)

        self._behind_torch(cur, prev, next, to_prev, to_next, out, weights, stats)
        _capi.check(self._lib.bbme_cells_temporal_filter_bgr_device(
            self._ctx, _ptr(prev), _ptr(cur), _ptr(next), cur.stride(0) if cur is not None else 0, _ptr(to_prev), _ptr(to_next),
            int(strength), win, _ptr(out), out.stride(0) if out is not None else 0, _ptr(weights),
            weights.stride(0) if weights is not None else 0, _ptr(stats), C.c_void_p(hip_stream_handle or 0)))
        return out, weights, stats

    # -- the colour frames along quarter-pel grids (the BGR SUBPEL TEMPORAL FILTER RULE of include/bbme.h) ----------------------
    def temporal_filter_subpel_bgr(self, strength, which=0, pair=0, out=None):
        """temporal_filter_bgr() at quarter-pel positions: the integer cells the frame's neighbours hang on are refined on the
        luma planes (subpel_cells) and each neighbour's 2x2 cell of the stored B,G,R frame is sampled bilinearly at its
        quarter-pel position; cost (the largest per-channel SAD of the rounded samples), weight and blend are
        temporal_filter_bgr()'s -> the UNPADDED (H, W, 3) uint8 frame."""
        return self._get_temporal_filtered(pair, which, strength, out, "temporal_filter_subpel_bgr", bgr=True, subpel=True)

    def temporal_filter_subpel_bgr_stats(self, strength, window=None):
        """temporal_filter_bgr_stats() of temporal_filter_subpel_bgr's frames: one dict(prev_cells, next_cells, weight, change)
        per frame of the context, from at most two refinement launches and one filter launch."""
        return self._temporal_filter_stats(strength, window, True, subpel=True)

    def cells_temporal_filter_subpel_bgr_device(self, cur, prev=None, next=None, q_to_prev=None, q_to_next=None, strength=64, out=None,
                                                weights=None, stats=None, window=None, stream=None):
        """The BGR subpel temporal filter rule on any three colour frames and any two quarter-pel grids in HBM: frames, out,
        weights and stats as in cells_temporal_filter_bgr_device; q_to_prev, q_to_next int16 CUDA tensors (CH, CW, 2) on cur with
        packed cells whose rows may be further apart than CW cells (what cells_subpel_device wrote, or a strided view), both
        with the same row pitch.  On the given HIP stream handle (default: the context's), ordered behind the context's stream;
        no host wait.  Needs neither frames nor an estimate."""
        import torch
        what = "cells_temporal_filter_subpel_bgr_device"
        ch, cw = self.cells_shape
        h, w = self.orig_height, self.orig_width
        for t in (cur, prev, next):
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3) and _packed_pixels(t)
                                      and cur is not None and t.stride(0) == cur.stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: colour frames must be uint8 CUDA tensors of shape (%d, %d, 3) with "
                                      "packed pixels and a common row pitch" % (what, h, w))
        grids = [t for t in (q_to_prev, q_to_next) if t is not None]
        for t in grids:
            if not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.stride(2) == 1 and t.stride(1) == 2
                    and t.stride(0) >= 2 * cw and t.stride(0) % 2 == 0 and t.data_ptr() % 4 == 0 and t.stride(0) == grids[0].stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: grids must be int16 CUDA tensors of shape (%d, %d, 2) with packed "
                                      "cells and rows a common whole number of cells apart" % (what, ch, cw))
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and _packed_pixels(out)):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d, 3) with packed pixels"
                                  % (what, h, w))
        if weights is not None and not (weights.is_cuda and weights.dtype == torch.uint8 and tuple(weights.shape) == (ch, cw)
                                        and weights.stride(1) == 1):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: weights must be a uint8 CUDA tensor of shape (%d, %d) with unit column "
                                  "stride" % (what, ch, cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 4
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 4" % what)
        win = _window(window)
        self._behind_torch(cur, prev, next, q_to_prev, q_to_next, out, weights, stats)
        _capi.check(self._lib.bbme_cells_subpel_temporal_filter_bgr_device(
            self._ctx, _ptr(prev), _ptr(cur), _ptr(next), cur.stride(0) if cur is not None else 0, _ptr(q_to_prev), _ptr(q_to_next),
            grids[0].stride(0) // 2 if grids else cw, int(strength), win, _ptr(out), out.stride(0) if out is not None else 0,
            _ptr(weights), weights.stride(0) if weights is not None else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, weights, stats

    # -- two frames on each side (the CELL COMPOSITION RULE and the WIDE TEMPORAL FILTER RULE of include/bbme.h) ----------------
    def _check_grid_tensor(self, t, what, name):
        """An int16 CUDA tensor (CH, CW, 2) of packed cells whose rows lie a whole number of cells apart -> that pitch in cells"""
        import torch
        ch, cw = self.cells_shape
        if not (t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 2) and t.stride(2) == 1 and t.stride(1) == 2
                and t.stride(0) >= 2 * cw and t.stride(0) % 2 == 0 and t.data_ptr() % 4 == 0):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: %s must be an int16 CUDA tensor of shape (%d, %d, 2) with packed cells and "
                                  "rows a whole number of cells apart" % (what, name, ch, cw))
        return t.stride(0) // 2

    def cells_compose_device(self, a, b, unit_shift=0, out=None, stats=None, window=None, stream=None):
        """The cell composition rule on any two grids in HBM: a (on X into Y) and b (on Y into Z) int16 CUDA tensors (CH, CW, 2),
        strided row views welcome; unit_shift 0 for pixels, 2 for quarter pels.  out: an int16 tensor of that shape that overlaps
        neither input, stats: an int64 or uint64 tensor of 2 (clamped, saturated over `window`), each optional, not both.  On
        the given HIP stream handle (default: the context's), ordered behind the context's stream; no host wait.  Needs neither
        frames nor an estimate."""
        import torch
        what = "cells_compose_device"
        pa, pb = self._check_grid_tensor(a, what, "a"), self._check_grid_tensor(b, what, "b")
        po = self._check_grid_tensor(out, what, "out") if out is not None else 0
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 2
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 2" % what)
        self._behind_torch(a, b, out, stats)
        _capi.check(self._lib.bbme_cells_compose_device(self._ctx, _ptr(a), pa, _ptr(b), pb, int(unit_shift), _window(window), _ptr(out),
                                                        po, _ptr(stats), C.c_void_p(stream or 0)))
        return out, stats

    def cells_temporal_filter_wide_device(self, cur, planes, grids, strength=64, out=None, weights=None, stats=None, window=None,
                                          stream=None):
        """The wide temporal filter rule on any planes and quarter-pel grids in HBM: cur a contiguous uint8 CUDA tensor
        (H_pad, W_pad); planes and grids sequences of four, P1, N1, P2, N2, None = absent: planes as cur, grids int16 (CH, CW, 2)
        on cur with one common row pitch (strided row views welcome).  out uint8 (H_pad, W_pad), weights int16 or uint16 (CH, CW)
        holding w_k << 4 k, both with unit column stride, stats an int64 or uint64 tensor of 6, each optional, not all three.  On
        the given HIP stream handle (default: the context's), ordered behind the context's stream; no host wait.  Needs neither
        frames nor an estimate."""
        import torch
        what = "cells_temporal_filter_wide_device"
        ch, cw = self.cells_shape
        h, w = self.padded_height, self.padded_width
        planes, grids = list(planes), list(grids)
        if len(planes) != 4 or len(grids) != 4:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: planes and grids are sequences of four (None = absent)" % what)
        for t in [cur] + planes:
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w) and t.is_contiguous()):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: planes must be contiguous uint8 CUDA tensors of shape (%d, %d)"
                                      % (what, h, w))
        pitches = {self._check_grid_tensor(t, what, "a grid") for t in grids if t is not None}
        if len(pitches) > 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: the grids' rows must lie a common number of cells apart" % what)
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w) and out.stride(1) == 1):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d) with unit column stride"
                                  % (what, h, w))
        if weights is not None and not (weights.is_cuda and weights.dtype in (torch.int16, torch.uint16) and tuple(weights.shape) == (ch, cw)
                                        and weights.stride(1) == 1):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: weights must be an int16 or uint16 CUDA tensor of shape (%d, %d) with unit "
                                  "column stride" % (what, ch, cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 6
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 6" % what)
        self._behind_torch(cur, *planes, *grids, out, weights, stats)
        _capi.check(self._lib.bbme_cells_wide_temporal_filter_device(
            self._ctx, _ptr4(planes), _ptr(cur), _ptr4(grids), pitches.pop() if pitches else cw, int(strength), _window(window),
            _ptr(out), out.stride(0) if out is not None else 0, _ptr(weights), weights.stride(0) if weights is not None else 0,
            _ptr(stats), C.c_void_p(stream or 0)))
        return out, weights, stats

    def cells_temporal_filter_wide_bgr_device(self, cur, frames, grids, strength=64, out=None, weights=None, stats=None, window=None,
                                              stream=None):
        """The BGR wide temporal filter rule on any colour frames and quarter-pel grids in HBM: cur a uint8 CUDA tensor (H, W, 3)
        with packed pixels (rows may be further apart than 3 W); frames and grids sequences of four, P1, N1, P2, N2, None =
        absent: frames as cur with its row pitch, grids int16 (CH, CW, 2) on cur with one common row pitch (strided row views
        welcome).  out uint8 (H, W, 3) with packed pixels, weights int16 or uint16 (CH, CW) holding w_k << 4 k with unit column
        stride, stats an int64 or uint64 tensor of 6, each optional, not all three.  On the given HIP stream handle (default: the
        context's), ordered behind the context's stream; no host wait.  Needs neither frames nor an estimate."""
        import torch
        what = "cells_temporal_filter_wide_bgr_device"
        ch, cw = self.cells_shape
        h, w = self.orig_height, self.orig_width
        frames, grids = list(frames), list(grids)
        if len(frames) != 4 or len(grids) != 4:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: frames and grids are sequences of four (None = absent)" % what)
        for t in [cur] + frames:
            if t is not None and not (t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == (h, w, 3) and _packed_pixels(t)
                                      and cur is not None and t.stride(0) == cur.stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "%s: colour frames must be uint8 CUDA tensors of shape (%d, %d, 3) with "
                                      "packed pixels and a common row pitch" % (what, h, w))
        pitches = {self._check_grid_tensor(t, what, "a grid") for t in grids if t is not None}
        if len(pitches) > 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: the grids' rows must lie a common number of cells apart" % what)
        if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (h, w, 3) and _packed_pixels(out)):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: out must be a uint8 CUDA tensor of shape (%d, %d, 3) with packed pixels"
                                  % (what, h, w))
        if weights is not None and not (weights.is_cuda and weights.dtype in (torch.int16, torch.uint16) and tuple(weights.shape) == (ch, cw)
                                        and weights.stride(1) == 1):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: weights must be an int16 or uint16 CUDA tensor of shape (%d, %d) with unit "
                                  "column stride" % (what, ch, cw))
        if stats is not None and not (stats.is_cuda and stats.dtype in (torch.int64, torch.uint64) and stats.numel() == 6
                                      and stats.is_contiguous()):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: stats must be a contiguous int64 or uint64 CUDA tensor of 6" % what)
        self._behind_torch(cur, *frames, *grids, out, weights, stats)
        _capi.check(self._lib.bbme_cells_wide_temporal_filter_bgr_device(
            self._ctx, _ptr4(frames), _ptr(cur), cur.stride(0) if cur is not None else 0, _ptr4(grids),
            pitches.pop() if pitches else cw, int(strength), _window(window), _ptr(out), out.stride(0) if out is not None else 0,
            _ptr(weights), weights.stride(0) if weights is not None else 0, _ptr(stats), C.c_void_p(stream or 0)))
        return out, weights, stats

    def frame_bgr_tensor(self, pair=0, which=0):
        """The stored colour frame `which` of `pair` in HBM (bbme_bgr_frames_device_pair) as a (H, W, 3) uint8 torch view; on an
        MFChain slot pair + which.  BbmeError (ERR_STATE) unless both frames of the pair have colour.  Read it only."""
        if which not in (0, 1):
            raise _capi.BbmeError(_capi.ERR_INVALID, "frame_bgr_tensor: which = %r (0 or 1)" % (which,))
        return self._hbm_view(self.bgr_frames_device_ptrs(pair)[int(which)], (self.orig_height, self.orig_width, 3), "|u1")

    def _hbm_view(self, ptr, shape, typestr):
        """A torch view of memory the context owns (no copy; valid while the context lives and holds what it held)."""
        import torch

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        return torch.as_tensor(v, device=torch.device("cuda", self.device))

    def frame_plane_tensor(self, pair=0, which=0):
        """The level-0 padded plane of frame `which` of `pair` in HBM (bbme_frame_plane_device) as a (H_pad, W_pad) uint8 torch
        view; on an MFChain slot pair + which.  Read it only: the context's estimates depend on it."""
        p = C.c_void_p()
        _capi.check(self._lib.bbme_frame_plane_device(self._ctx, pair, int(which), 0, C.byref(p)))
        return self._hbm_view(p.value, (self.padded_height, self.padded_width), "|u1")

    def cells_tensor(self, pair=0):
        """The forward 2x2-cell grid of `pair` in HBM as a (CH, CW, 2) int16 torch view."""
        p = C.c_void_p()
        _capi.check(self._lib.bbme_cells_device_pair(self._ctx, pair, C.byref(p)))
        return self._hbm_view(p.value, self.cells_shape + (2,), "<i2")

    def backward_cells_tensor(self, pair=0):
        """The backward 2x2-cell grid of `pair` in HBM after estimate_bidirectional_async() as a (CH, CW, 2) int16 torch view."""
        return self._hbm_view(self.backward_cells_device_ptr(pair), self.cells_shape + (2,), "<i2")

    def calcMotionBlockMatchingSubsampled(self, scale=None):
        """calcMotionBlockMatching followed by get_subsampled_flow: nothing dense crosses PCIe."""
        self.estimate_async()
        return self.get_subsampled_flow(scale)

    def get_cells(self, out=None):
        shape = (self.padded_height // 2, self.padded_width // 2, 2)
        out = _host_out(out, shape, np.int16, "get_cells")
        _capi.check(self._lib.bbme_get_cells_host(self._ctx, out.ctypes.data))
        return out

    def flow_device_ptr(self):
        p = C.c_void_p()
        _capi.check(self._lib.bbme_flow_device(self._ctx, C.byref(p)))
        return p.value

    def cells_device_ptr(self):
        p = C.c_void_p()
        _capi.check(self._lib.bbme_cells_device(self._ctx, C.byref(p)))
        return p.value

    def expand_cells_device(self, cells_ptr, flow_ptr, hip_stream_handle=None):
        """copy_to_all_pixels for a cell grid anywhere in HBM -> dense padded field (device pointers), on the
        context's stream or on the given HIP stream."""
        _capi.check(self._lib.bbme_expand_cells_device_on(self._ctx, C.c_void_p(cells_ptr), C.c_void_p(flow_ptr),
                                                          C.c_void_p(hip_stream_handle or 0)))

    def calculate_mse_device(self, gtruth, scale=4):
        """Flow::CalculateMSE against a ground-truth field already in HBM (torch float32 CUDA tensor (h, w, 2)),
        fused with the driver's every-`scale`-th-pixel / `scale` subsampling; nothing is downloaded but the sums."""
        assert gtruth.is_cuda and gtruth.is_contiguous() and gtruth.dim() == 3 and gtruth.shape[2] == 2
        assert gtruth.dtype.itemsize == 4 and gtruth.dtype.is_floating_point
        out = C.c_double()
        self._behind_torch(gtruth)
        _capi.check(self._lib.bbme_calculate_mse_device(self._ctx, C.c_void_p(gtruth.data_ptr()), gtruth.shape[1],
                                                        gtruth.shape[0], int(scale), C.byref(out)))
        return out.value

    def calcMotionBlockMatching(self):
        """cv::Mat MF::calcMotionBlockMatching() -- dense padded (H, W, 2) float32 (u, v) field."""
        self.estimate_async()
        return self.get_flow()

    # -- the reference's private methods, one stage at a time (parity tests) --------------
    def stage_search(self, level):
        """copyMVs() + calcLevelBM() of one level."""
        _capi.check(self._lib.bbme_stage_search(self._ctx, level))

    def stage_regularize(self, level, block, lambda_multiplier):
        """One regularize_MVs() sweep (divide_blocks() first when the grid is at 2*block)."""
        _capi.check(self._lib.bbme_stage_regularize(self._ctx, level, block, lambda_multiplier))

    def stage_get_mvs(self, level, block):
        w, h, _, _ = self.level_geometry(level)
        out = np.empty((h // block, w // block, 2), np.int16)
        _capi.check(self._lib.bbme_stage_get_mvs(self._ctx, level, block, out.ctypes.data))
        return out

    def stage_set_mvs(self, level, block, mvs):
        w, h, _, _ = self.level_geometry(level)
        mvs = np.ascontiguousarray(mvs, np.int16)
        assert mvs.shape == (h // block, w // block, 2)
        _capi.check(self._lib.bbme_stage_set_mvs(self._ctx, level, block, mvs.ctypes.data))

    def stage_expand(self):
        _capi.check(self._lib.bbme_stage_expand(self._ctx))

    def fixup_counts(self, pair=0):
        """Blocks per level that the last estimate searched again behind a speculative search (bbme_fixup_counts): 0 for a level
        whose search was not speculative.  Waits for the estimate."""
        v = (C.c_uint * self.num_levels)()
        _capi.check(self._lib.bbme_fixup_counts(self._ctx, pair, v, self.num_levels))
        return list(v)

    def last_sweep_passes(self):
        v = (C.c_int * 2)()
        _capi.check(self._lib.bbme_last_sweep_passes(self._ctx, v))
        return v[0], v[1]

    def sweep_stats(self):
        v = (C.c_uint * 16)()
        _capi.check(self._lib.bbme_sweep_stats(self._ctx, v))
        return list(v)

    def set_profiling(self, enabled):
        _capi.check(self._lib.bbme_set_profiling(self._ctx, int(enabled)))

    def timings(self):
        v = [C.c_float() for _ in range(5)]
        _capi.check(self._lib.bbme_get_timings(self._ctx, *[C.byref(x) for x in v]))
        return dict(zip(("total_ms", "search_ms", "regularize_ms", "expand_ms", "search_level0_ms"),
                        [x.value for x in v]))


class MFBatch(MF):
    """Several independent frame pairs of one size behind ONE launch sequence (bbme_create_batch): the pairs of a sequence
    that share a GPU.  Every kernel of the estimate works on all pairs at once; each pair's field is bit for bit what an MF
    of its own returns.  `pairs` = [(image1, image2), ...] host arrays, or torch uint8 CUDA tensors with
    frames_on_device=True.  Of the methods inherited from MF, set_frames, set_frames_device, get_flow, get_cells,
    get_subsampled_flow, draw_MVimage, compensation_error and the device-pointer getters address pair 0; the single-pair calls (stage_*, the level planes,
    last_sweep_passes, sweep_stats, calculate_mse_device) raise BbmeError (ERR_UNSUPPORTED) on a batch of more than one pair.
    upsample=4: the pairs are original frames, up-sampled x4 on the GPU, as MF(..., upsample=4)."""

    def __init__(self, pairs, search_size, block_size, num_levels=None, device=0, frames_on_device=False, upsample=1):
        self.upsample = _check_upsample(upsample)
        if num_levels is None:
            num_levels = len(block_size)
        if num_levels <= 0 or not pairs:
            raise _capi.BbmeError(_capi.ERR_INVALID, "num_levels must be > 0 and pairs non-empty")
        self._ctx = C.c_void_p()
        self._lib = _capi.lib()
        self.device = device
        self.batch = len(pairs)
        self._torch_frames = [None] * self.batch
        h, w = pairs[0][0].shape[:2]
        self.source_height, self.source_width = h, w
        self.orig_height, self.orig_width = h * upsample, w * upsample
        self.params = _capi.make_params(list(search_size)[:num_levels], list(block_size)[:num_levels])
        _capi.check(self._lib.bbme_create_batch(C.byref(self.params), self.orig_width, self.orig_height, device, self.batch,
                                                C.byref(self._ctx)))
        pw, ph, px, py = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _capi.check(self._lib.bbme_get_geometry(self._ctx, C.byref(pw), C.byref(ph), C.byref(px), C.byref(py)))
        self.padded_width, self.padded_height = pw.value, ph.value
        self.padding_x, self.padding_y = px.value, py.value
        self.num_levels = num_levels
        for p, (image1, image2) in enumerate(pairs):
            if frames_on_device:
                self.set_pair_device(p, image1, image2)
            else:
                self.set_pair(p, image1, image2)

    def set_pair(self, pair, image1, image2):
        self._set_host_pair(pair, image1, image2)

    def set_frames(self, image1, image2):
        """Pair 0 (the inherited entry point without a pair index)."""
        self.set_pair(0, image1, image2)

    def set_frames_device(self, image1, image2):
        """Pair 0 (the inherited entry point without a pair index)."""
        self.set_pair_device(0, image1, image2)

    def set_pair_device(self, pair, image1, image2):
        if not 0 <= pair < self.batch:
            raise _capi.BbmeError(_capi.ERR_INVALID, "pair %d of a batch of %d" % (pair, self.batch))
        self._set_device_pair(pair, image1, image2)
        self._torch_frames[pair] = (image1, image2)

    def get_pair_flow(self, pair, out=None):
        shape = (self.padded_height, self.padded_width, 2)
        out = _host_out(out, shape, np.float32, "get_pair_flow")
        _capi.check(self._lib.bbme_get_flow_host_pair(self._ctx, pair, out.ctypes.data))
        return out

    def get_pair_cells(self, pair, out=None):
        shape = (self.padded_height // 2, self.padded_width // 2, 2)
        out = _host_out(out, shape, np.int16, "get_pair_cells")
        _capi.check(self._lib.bbme_get_cells_host_pair(self._ctx, pair, out.ctypes.data))
        return out

    def get_pair_subsampled_flow(self, pair, scale=None, out=None):
        """MF.get_subsampled_flow of one pair."""
        return self._get_subsampled(pair, scale, out, "get_pair_subsampled_flow")

    def get_pair_motion_compensated(self, pair, level=0, block=2, fill=0, out=None):
        """MF.draw_MVimage of one pair."""
        return self._get_motion_compensated(pair, level, block, fill, out, "get_pair_motion_compensated")

    def get_pair_backward_cells(self, pair, out=None):
        """MF.get_backward_cells of one pair."""
        return self._get_backward_cells(pair, out, "get_pair_backward_cells")

    def get_pair_subpel_cells(self, pair, which="forward", out=None):
        """Pair `pair`'s cells refined to quarter-pel -> (CH, CW, 2) int16 (MF.subpel_cells)."""
        return self._subpel_cells(pair, which, out, "get_pair_subpel_cells")

    def get_pair_subpel_flow(self, pair, which="forward", out=None):
        """Pair `pair`'s refined field of the unpadded source frame -> (H, W, 2) float32 (MF.subpel_flow)."""
        return self._subpel_flow(pair, which, out, "get_pair_subpel_flow")

    def subpel_stats_all(self, which="forward", window=None):
        """MF.subpel_stats of every pair, from one launch -> list of dicts."""
        return self._subpel_stats(which, window)

    def get_pair_motion_compensated_subpel(self, pair, which="forward", fill=0, out=None):
        """MF.draw_MVimage_subpel of one pair."""
        return self._get_subpel_compensated(pair, which, fill, out, "get_pair_motion_compensated_subpel")

    def compensation_errors_subpel(self, which="forward", window=None):
        """MF.compensation_error_subpel of every pair, in order, from one refinement and one compensation launch."""
        return self._subpel_compensation_stats(which, window)

    def global_motion_all(self, which="forward", subpel=False, kind="affine", tol=1.0, iterations=3, mask_tol=None, window=None,
                          maps=False):
        """MF.global_motion of every pair, in order, from one launch per step -> list of dicts; maps=True adds each pair's map
        (one more launch and download per pair)."""
        out = self._global_motion(which, subpel, kind, tol, iterations, mask_tol, window)
        if maps:
            for p, d in enumerate(out):
                d["map"] = self._global_motion_map(p, which, subpel, mask_tol, d["model"], tol, None, "global_motion_all")
        return out

    def get_pair_global_compensated(self, pair, model, unit=1, which="forward", fill=0, out=None):
        """MF.draw_MVimage_global of one pair."""
        return self._get_global_compensated(pair, which, model, unit, fill, out, "get_pair_global_compensated")

    def compensation_errors_global(self, models, unit=1, which="forward", window=None):
        """MF.compensation_error_global of every pair under its own model (models: (pairs, 6) int32), from one launch."""
        return self._global_compensation_stats(which, models, unit, window)

    def get_pair_global_compensated_bgr(self, pair, model, unit=1, which="forward", fill=0, out=None):
        """MF.draw_MVimage_global_bgr of one pair."""
        return self._get_global_compensated_bgr(pair, which, model, unit, fill, out, "get_pair_global_compensated_bgr")

    def compensation_errors_global_bgr(self, models, unit=1, which="forward", window=None):
        """MF.compensation_error_global_bgr of every pair under its own model (models: (pairs, 6) int32), from one launch."""
        return self._global_compensation_stats_bgr(which, models, unit, window)

    def get_pair_motion_compensated_bgr(self, pair, unit=4, which="forward", fill=0, out=None):
        """MF.draw_MVimage_subpel_bgr (unit=4) or MF.draw_MVimage_bgr (unit=1) of one pair."""
        return self._get_compensated_bgr(pair, which, unit, fill, out, "get_pair_motion_compensated_bgr")

    def compensation_errors_bgr(self, unit=4, which="forward", window=None):
        """MF.compensation_error_subpel_bgr (unit=4) or MF.compensation_error_bgr (unit=1) of every pair, in order, from one
        refinement launch (unit 4 only) and one compensation launch."""
        return self._compensation_stats_bgr(which, unit, window)

    def consistency_stats_all(self, which="forward", tol=1, window=None):
        """MF.consistency_stats of every pair, in order, from one launch."""
        return self._consistency_stats(which, tol, window)

    def get_pair_flow_color(self, pair, scale=None, maxmotion=-1.0, which="forward", out=None):
        """MF.flow_color of one pair."""
        return self._get_flow_color(pair, scale, maxmotion, which, out, "get_pair_flow_color")

    def flow_ranges_all(self, which="forward", scale=None):
        """MF.flow_range of every pair from one launch -> (pairs, 5) float32; a video is coloured with one common maxmotion
        by passing flow_ranges_all()[:, 0].max() to get_pair_flow_color."""
        return self._flow_ranges(which, scale)

    def get_pair_interpolated(self, pair, num=1, den=2, out=None):
        """MF.interpolate of one pair."""
        return self._get_interpolated(pair, num, den, out, "get_pair_interpolated")

    def interpolation_stats_all(self, num=1, den=2, window=None):
        """MF.interpolation_stats of every pair, in order, from one launch."""
        return self._interpolation_stats(num, den, window)

    def get_pair_interpolated_subpel(self, pair, num=1, den=2, out=None):
        """MF.interpolate_subpel of one pair."""
        return self._get_interpolated(pair, num, den, out, "get_pair_interpolated_subpel", subpel=True)

    def get_pair_interpolated_subpel_bgr(self, pair, num=1, den=2, out=None):
        """MF.interpolate_subpel_bgr of one pair."""
        return self._get_interpolated(pair, num, den, out, "get_pair_interpolated_subpel_bgr", bgr=True, subpel=True)

    def interpolation_stats_subpel_all(self, num=1, den=2, window=None):
        """MF.interpolation_stats_subpel of every pair, in order, from two refinement launches and one interpolation launch."""
        return self._interpolation_stats(num, den, window, subpel=True)

    def get_frame_filtered(self, pair, which, strength, out=None):
        """MF.temporal_filter of frame `which` of one pair."""
        return self._get_temporal_filtered(pair, which, strength, out, "get_frame_filtered")

    def get_frame_filtered_bgr(self, pair, which, strength, out=None):
        """MF.temporal_filter_bgr of frame `which` of one pair."""
        return self._get_temporal_filtered(pair, which, strength, out, "get_frame_filtered_bgr", bgr=True)

    def get_frame_filtered_subpel(self, pair, which, strength, out=None):
        """MF.temporal_filter_subpel of frame `which` of one pair."""
        return self._get_temporal_filtered(pair, which, strength, out, "get_frame_filtered_subpel", subpel=True)

    def get_frame_filtered_subpel_bgr(self, pair, which, strength, out=None):
        """MF.temporal_filter_subpel_bgr of frame `which` of one pair."""
        return self._get_temporal_filtered(pair, which, strength, out, "get_frame_filtered_subpel_bgr", bgr=True, subpel=True)

    def compensation_errors(self, level=0, block=2, window=None):
        """MF.compensation_error of every pair, in order, from one launch."""
        return self._compensation_stats(level, block, window)

    def calcMotionBlockMatching(self):
        """Every pair's dense padded field, in order."""
        self.estimate_async()
        return [self.get_pair_flow(p) for p in range(self.batch)]


class MFChain(MFBatch):
    """The CONSECUTIVE pairs of a video behind one launch sequence (bbme_create_chain): `frames` = [f0, f1, ..., fP] are P + 1
    frame slots and pair p = (f_p, f_p+1), so batch = len(frames) - 1 and every frame is uploaded, padded (or up-sampled) and
    run through the pyramid ONCE -- an MFBatch fed the same pairs does all of that twice for every inner frame.  Each pair's
    field is bit for bit what MF(f_p, f_p+1, ...) returns.  Frames are host arrays, or torch uint8 CUDA tensors with
    frames_on_device=True; upsample=4: original frames, up-sampled x4 on the GPU.

        chain = MFChain(video[0:P + 1], search, block)       # pairs 0 .. P-1
        chain.estimate_async(); cells = [chain.get_pair_cells(p) for p in range(P)]
        chain.advance(video[P + 1:2 * P + 1])                 # slot P -> slot 0 on the GPU, then P new frames: pairs P .. 2P-1

    The get_pair_* getters, compensation_errors, estimate_async and the switches are MFBatch's.  The pair setters (set_pair,
    set_frames, ...) raise BbmeError (ERR_UNSUPPORTED): a plane here belongs to two pairs and is set by slot."""

    def __init__(self, frames, search_size, block_size, num_levels=None, device=0, frames_on_device=False, upsample=1):
        self.upsample = _check_upsample(upsample)
        if num_levels is None:
            num_levels = len(block_size)
        frames = list(frames)
        if num_levels <= 0 or len(frames) < 2:
            raise _capi.BbmeError(_capi.ERR_INVALID, "num_levels must be > 0 and a chain needs at least two frames")
        self._ctx = C.c_void_p()
        self._lib = _capi.lib()
        self.device = device
        self.batch = len(frames) - 1
        self.frames_on_device = bool(frames_on_device)
        self._torch_frames = [None] * len(frames)
        h, w = frames[0].shape[:2]
        self.source_height, self.source_width = h, w
        self.orig_height, self.orig_width = h * upsample, w * upsample
        self.params = _capi.make_params(list(search_size)[:num_levels], list(block_size)[:num_levels])
        _capi.check(self._lib.bbme_create_chain(C.byref(self.params), self.orig_width, self.orig_height, device, self.batch,
                                                C.byref(self._ctx)))
        pw, ph, px, py = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _capi.check(self._lib.bbme_get_geometry(self._ctx, C.byref(pw), C.byref(ph), C.byref(px), C.byref(py)))
        self.padded_width, self.padded_height = pw.value, ph.value
        self.padding_x, self.padding_y = px.value, py.value
        self.num_levels = num_levels
        self.set_frame_run(0, frames)

    @property
    def slots(self):
        n = C.c_int()
        _capi.check(self._lib.bbme_chain_frames(self._ctx, C.byref(n)))
        return n.value

    def set_frame_run(self, first, frames, wait=True):
        """Slots first .. first + len(frames) - 1 from `frames`: host arrays (wait=False only enqueues the uploads: the arrays,
        pinned for a truly asynchronous copy, must stay untouched until the context's stream has passed them), or torch uint8
        CUDA tensors on a context made with frames_on_device=True (ordered behind torch's current stream, kept referenced)."""
        frames = list(frames)
        n = len(frames)
        if n < 1 or first < 0 or first + n > self.batch + 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "slots %d .. %d of a chain of %d" % (first, first + n - 1, self.batch + 1))
        table = (C.c_void_p * n)()
        if self.frames_on_device:
            import torch
            self._check_device_run(frames)
            for i, t in enumerate(frames):
                table[i] = t.data_ptr()
            _capi.check(self._lib.bbme_wait_for_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(frames[0].device).cuda_stream)))
            if frames[0].dim() == 3:
                _capi.check(self._lib.bbme_set_chain_frames_device_bgr(self._ctx, first, n, table, frames[0].stride(0)))
            else:
                _capi.check(self._lib.bbme_set_chain_frames_device(self._ctx, first, n, table, frames[0].stride(0), self.upsample))
            self._torch_frames[first:first + n] = frames
            return
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        for i, f in enumerate(frames):
            if f.shape not in self._frame_shapes() or f.shape != frames[0].shape:
                raise _capi.BbmeError(_capi.ERR_INVALID, "frames must keep the size the context was created for, all grey or all colour")
            table[i] = f.ctypes.data
        if frames[0].ndim == 3:
            setter = self._lib.bbme_set_chain_frames_host_bgr if wait else self._lib.bbme_set_chain_frames_host_bgr_async
            _capi.check(setter(self._ctx, first, n, table, 3 * self.source_width))
        else:
            setter = self._lib.bbme_set_chain_frames_host if wait else self._lib.bbme_set_chain_frames_host_async
            _capi.check(setter(self._ctx, first, n, table, self.source_width, self.upsample))
        if not wait:
            self._host_frames_in_flight = frames          # keeps converted copies alive until the next run replaces them

    def _temporal_filter_run(self, strength, first, count, what, bgr, subpel=False):
        import torch
        first = int(first)
        count = self.batch + 1 - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.batch + 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: slots %d .. %d of a chain of %d" % (what, first, first + count - 1, self.batch + 1))
        frames = torch.empty((count,) + self._out_shape(bgr), dtype=torch.uint8, device="cuda:%d" % self.device)
        self._behind_torch(frames)
        run = self._lib.bbme_temporal_filter_bgr_chain_device if bgr else self._lib.bbme_temporal_filter_chain_device
        if subpel:
            run = self._lib.bbme_subpel_temporal_filter_bgr_chain_device if bgr else self._lib.bbme_subpel_temporal_filter_chain_device
        _capi.check(run(self._ctx, first, count, int(strength), _ptr(frames), frames.stride(1), frames.stride(0), None))
        self.synchronize()
        return frames.cpu().numpy()

    def temporal_filter_run(self, strength, first=0, count=None):
        """Slots first .. first + count - 1 (default: to the last) filtered from one launch -> (count, H_pad, W_pad) uint8: the
        first slot of the chain has no previous and the last no next neighbour, every other slot uses both."""
        return self._temporal_filter_run(strength, first, count, "temporal_filter_run", False)

    def temporal_filter_run_subpel(self, strength, first=0, count=None):
        """temporal_filter_run() at quarter-pel positions (MF.temporal_filter_subpel): at most two refinement launches for the
        cells the run reads, then one filter launch -> (count, H_pad, W_pad) uint8."""
        return self._temporal_filter_run(strength, first, count, "temporal_filter_run_subpel", False, subpel=True)

    def temporal_filter_run_subpel_bgr(self, strength, first=0, count=None):
        """temporal_filter_run_bgr() at quarter-pel positions (MF.temporal_filter_subpel_bgr): at most two refinement launches on
        the luma planes for the cells the run reads, then one filter launch -> (count, H, W, 3) uint8, unpadded."""
        return self._temporal_filter_run(strength, first, count, "temporal_filter_run_subpel_bgr", True, subpel=True)

    def temporal_filter_run_bgr(self, strength, first=0, count=None):
        """temporal_filter_run() in colour: the stored B,G,R frames of slots first .. first + count - 1 (default: to the last)
        filtered from one launch -> (count, H, W, 3) uint8, unpadded."""
        return self._temporal_filter_run(strength, first, count, "temporal_filter_run_bgr", True)

    # -- two frames on each side (the CELL COMPOSITION RULE and the WIDE TEMPORAL FILTER RULE of include/bbme.h) ----------------
    def composed_cells(self, f, side):
        """The integer grid on slot f into slot f + 2 (side = +1: the forward cells of pair f composed with those of pair f + 1)
        or into slot f - 2 (side = -1: the backward cells of pair f - 1 with those of pair f - 2), after
        estimate_bidirectional_async -> (CH, CW, 2) int16."""
        import torch
        ch, cw = self.cells_shape
        out = torch.empty((ch, cw, 2), dtype=torch.int16, device="cuda:%d" % self.device)
        self._behind_torch(out)
        _capi.check(self._lib.bbme_compose_chain_device(self._ctx, int(f), 1, int(side), _ptr(out), cw, 0, None))
        self.synchronize()
        return out.cpu().numpy()

    def temporal_filter_run_wide(self, strength, first=0, count=None):
        """Slots first .. first + count - 1 (default: to the last) filtered over two frames on each side, as far as the chain
        has them (the wide temporal filter rule): the grids into slots f +- 1 are temporal_filter_run_subpel's, those into slots
        f +- 2 composed_cells refined against the real frame pair; one filter launch -> (count, H_pad, W_pad) uint8."""
        import torch
        first = int(first)
        count = self.batch + 1 - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.batch + 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "temporal_filter_run_wide: slots %d .. %d of a chain of %d"
                                  % (first, first + count - 1, self.batch + 1))
        frames = torch.empty((count,) + self._out_shape(False), dtype=torch.uint8, device="cuda:%d" % self.device)
        self._behind_torch(frames)
        _capi.check(self._lib.bbme_wide_temporal_filter_chain_device(self._ctx, first, count, int(strength), _ptr(frames),
                                                                     frames.stride(1), frames.stride(0), None))
        self.synchronize()
        return frames.cpu().numpy()

    def get_frame_filtered_wide(self, f, strength, out=None):
        """Slot f alone as temporal_filter_run_wide filters it -> the padded (H_pad, W_pad) uint8 plane."""
        out = _host_out(out, self._out_shape(False), np.uint8, "get_frame_filtered_wide")
        _capi.check(self._lib.bbme_get_wide_temporal_filtered_host(self._ctx, int(f), int(strength), out.ctypes.data))
        return out

    def temporal_filter_wide_stats(self, strength, window=None):
        """One dict(prev1_cells, next1_cells, prev2_cells, next2_cells, weight, change) per slot of the chain over `window` in
        cells, from one filter launch."""
        slots = self.batch + 1
        s = (C.c_ulonglong * (6 * slots))()
        _capi.check(self._lib.bbme_wide_temporal_filter_stats(self._ctx, int(strength), self._stats_window(window), s))
        return [dict(zip(WIDE_STAT_KEYS, s[6 * f:6 * f + 6])) for f in range(slots)]

    def temporal_filter_run_wide_bgr(self, strength, first=0, count=None):
        """temporal_filter_run_wide() in colour (the BGR wide temporal filter rule): the same grids, made on the luma planes, then
        one filter launch on the stored B,G,R frames -> (count, H, W, 3) uint8, unpadded."""
        import torch
        first = int(first)
        count = self.batch + 1 - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.batch + 1:
            raise _capi.BbmeError(_capi.ERR_INVALID, "temporal_filter_run_wide_bgr: slots %d .. %d of a chain of %d"
                                  % (first, first + count - 1, self.batch + 1))
        frames = torch.empty((count,) + self._out_shape(True), dtype=torch.uint8, device="cuda:%d" % self.device)
        self._behind_torch(frames)
        _capi.check(self._lib.bbme_wide_temporal_filter_bgr_chain_device(self._ctx, first, count, int(strength), _ptr(frames),
                                                                         frames.stride(1), frames.stride(0), None))
        self.synchronize()
        return frames.cpu().numpy()

    def get_frame_filtered_wide_bgr(self, f, strength, out=None):
        """Slot f alone as temporal_filter_run_wide_bgr filters it -> the (H, W, 3) uint8 frame."""
        out = _host_out(out, self._out_shape(True), np.uint8, "get_frame_filtered_wide_bgr")
        _capi.check(self._lib.bbme_get_wide_temporal_filtered_bgr_host(self._ctx, int(f), int(strength), out.ctypes.data))
        return out

    def temporal_filter_wide_bgr_stats(self, strength, window=None):
        """temporal_filter_wide_stats() of the colour filter: one dict per slot of the chain over `window` in cells, from one
        filter launch; change is summed over three channels."""
        slots = self.batch + 1
        s = (C.c_ulonglong * (6 * slots))()
        _capi.check(self._lib.bbme_wide_temporal_filter_bgr_stats(self._ctx, int(strength), self._stats_window(window), s))
        return [dict(zip(WIDE_STAT_KEYS, s[6 * f:6 * f + 6])) for f in range(slots)]

    def get_slot_plane(self, level, slot):
        """The padded plane of frame slot `slot` at `level` (bbme_get_chain_plane_host) -> (level height, level width) uint8."""
        w, h, _, _ = self.level_geometry(level)
        out = np.empty((h, w), np.uint8)
        _capi.check(self._lib.bbme_get_chain_plane_host(self._ctx, level, slot, out.ctypes.data))
        return out

    def _check_device_run(self, frames):
        import torch
        for t in frames:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) in self._frame_shapes()
                    and t.shape == frames[0].shape and _packed_pixels(t) and t.stride(0) == frames[0].stride(0)):
                raise _capi.BbmeError(_capi.ERR_INVALID, "device frames must be uint8 CUDA tensors of %d x %d (or, all of them, "
                                      "%d x %d x 3 in B,G,R order) with packed pixels and a common row pitch"
                                      % (self.source_height, self.source_width, self.source_height, self.source_width))

    def advance(self, new_frames, wait=True):
        """The next round of the video: the last slot becomes slot 0 on the GPU (bbme_chain_advance: one copy launch, nothing
        re-uploaded or re-computed), then `new_frames` go into slots 1 .. (all `batch` of them before the next estimate)."""
        _capi.check(self._lib.bbme_chain_advance(self._ctx))
        self._torch_frames = [self._torch_frames[-1]] + [None] * self.batch
        new_frames = list(new_frames)
        if new_frames:
            self.set_frame_run(1, new_frames, wait=wait)


def _is_frame_shape(shape):
    """(H, W) grey or (H, W, 3) B,G,R."""
    return len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)


def _packed_pixels(t):
    """A frame tensor whose pixels lie side by side in a row: unit column stride (grey), or 3 bytes per pixel (B,G,R)."""
    return t.stride(1) == 1 if t.dim() == 2 else (t.stride(2) == 1 and t.stride(1) == 3)


def _which(which):
    if which in ("forward", 0, False):
        return 0
    if which in ("backward", 1, True):
        return 1
    raise _capi.BbmeError(_capi.ERR_INVALID, "which must be 'forward' or 'backward', not %r" % (which,))


_SUBPEL_STATS = ("valid", "moved", "cost_integer", "cost_refined")


def subpel_cells(image1, image2, cells, window=None):
    """The subpel rule of include/bbme.h on the CPU (bbme_subpel_host): image1, image2 uint8 (H, W) planes (both even), cells an
    int16 (H / 2, W / 2, 2) grid of integer vectors on image1 into image2 -> (quarter-pel grid (H / 2, W / 2, 2) int16,
    dict(valid, moved, cost_integer, cost_refined) over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    image1 = np.ascontiguousarray(image1, np.uint8)
    image2 = np.ascontiguousarray(image2, np.uint8)
    cells = np.ascontiguousarray(cells, np.int16)
    if image1.ndim != 2 or image1.shape != image2.shape or cells.shape != (image1.shape[0] // 2, image1.shape[1] // 2, 2):
        raise _capi.BbmeError(_capi.ERR_INVALID, "subpel_cells: two uint8 planes of one shape (H, W) and an int16 grid (H / 2, W / 2, 2)")
    h, w = image1.shape
    out = np.empty(cells.shape, np.int16)
    s = (C.c_ulonglong * 4)()
    _capi.check(_capi.lib().bbme_subpel_host(image1.ctypes.data, image2.ctypes.data, w, h, cells.ctypes.data, _window(window),
                                             out.ctypes.data, s))
    return out, dict(zip(_SUBPEL_STATS, list(s)))


def _residual_dict(s, channels=1):
    """dict(sse, sad, pixels, skipped, mse, psnr) of the four residual statistics of a compensation rule; sse is summed over
    `channels` samples per pixel."""
    sse, sad, pixels, skipped = s
    mse = sse / (channels * pixels) if pixels else math.nan
    psnr = math.nan if not pixels else math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * channels * pixels / sse)
    return dict(sse=sse, sad=sad, pixels=pixels, skipped=skipped, mse=mse, psnr=psnr)


def compensate_cells_subpel(image1, image2, q4, fill=0, window=None):
    """The subpel compensation rule of include/bbme.h on the CPU (bbme_subpel_compensate_host): image1, image2 uint8 (H, W)
    planes (both even), q4 an int16 (H / 2, W / 2, 2) grid of quarter-pel vectors on image1 into image2 (subpel_cells' output)
    -> (compensated plane (H, W) uint8, dict(sse, sad, pixels, skipped, mse, psnr) against image1 over window (x0, y0, w, h)
    in pixels, None = the whole plane)."""
    image1 = np.ascontiguousarray(image1, np.uint8)
    image2 = np.ascontiguousarray(image2, np.uint8)
    q4 = np.ascontiguousarray(q4, np.int16)
    if image1.ndim != 2 or image1.shape != image2.shape or q4.shape != (image1.shape[0] // 2, image1.shape[1] // 2, 2):
        raise _capi.BbmeError(_capi.ERR_INVALID, "compensate_cells_subpel: two uint8 planes of one shape (H, W) and an int16 grid "
                                                 "(H / 2, W / 2, 2)")
    h, w = image1.shape
    out = np.empty((h, w), np.uint8)
    s = (C.c_ulonglong * 4)()
    _capi.check(_capi.lib().bbme_subpel_compensate_host(image1.ctypes.data, image2.ctypes.data, w, h, q4.ctypes.data, int(fill),
                                                        _window(window), out.ctypes.data, s))
    return out, _residual_dict(list(s))


GM_TRANSLATION, GM_AFFINE = 0, 1                          # `kind` of the global motion rule
GM_INLIER, GM_OUTLIER, GM_EXCLUDED = 0, 1, 2             # classes of a global motion map
GM_BINS = 2048
GM_STAT_KEYS = ("inliers", "outliers", "excluded", "residual", "sum_x", "sum_y", "sum_xx", "sum_xy", "sum_yy", "sum_dx", "sum_dy",
                "sum_x_dx", "sum_y_dx", "sum_x_dy", "sum_y_dy", "sum_sq")


def _gm_kind(kind):
    if kind in ("translation", GM_TRANSLATION):
        return GM_TRANSLATION
    if kind in ("affine", GM_AFFINE):
        return GM_AFFINE
    raise _capi.BbmeError(_capi.ERR_INVALID, "kind must be 'translation' or 'affine', not %r" % (kind,))


def _gm_tol(tol, unit):
    """A tolerance in pixels as Q16 grid units of 1 / unit pixel."""
    return int(round(float(tol) * unit * 65536.0))


def _gm_model(model, what):
    model = np.ascontiguousarray(model, np.int32).reshape(-1)
    if model.size != 6:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: a model is six int32" % what)
    return model


def _gm_dict(model, words, unit):
    model = np.array(model, np.int32)
    return dict(model=model, unit=unit, translation=(model[0] / 65536.0 / unit, model[3] / 65536.0 / unit),
                statistics=dict(zip(GM_STAT_KEYS, [int(v) for v in words])))


def _gm_grid(cells, exclude, what):
    """(cells, exclude, exclude pitch, cw, ch) of a grid and its optional exclusion mask, whose rows may be strided."""
    cells = np.ascontiguousarray(cells, np.int16)
    if cells.ndim != 3 or cells.shape[2] != 2:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: an int16 grid (CH, CW, 2)" % what)
    ch, cw = cells.shape[:2]
    pitch = 0
    if exclude is not None:
        exclude = np.asarray(exclude, np.uint8)
        if exclude.shape != (ch, cw) or exclude.strides[1] != 1 or exclude.strides[0] < cw:
            exclude = np.ascontiguousarray(exclude)
        if exclude.shape != (ch, cw):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: exclude must be a uint8 array (%d, %d)" % (what, ch, cw))
        pitch = exclude.strides[0]
    return cells, exclude, pitch, cw, ch


def vector_histogram_cells(cells, exclude=None, window=None):
    """The histogram part of the global motion rule on the CPU (bbme_vector_histogram_host): cells an int16 (CH, CW, 2) grid,
    exclude a uint8 (CH, CW) mask (non-zero = excluded) or None -> (2, 2048) uint32, row 0 for dx, row 1 for dy, over window
    (cx0, cy0, cw, ch) in cells, None = all cells."""
    cells, exclude, pitch, cw, ch = _gm_grid(cells, exclude, "vector_histogram_cells")
    hist = np.empty((2, GM_BINS), np.uint32)
    _capi.check(_capi.lib().bbme_vector_histogram_host(cells.ctypes.data, cw, ch, _ptr(exclude), pitch, _window(window), hist.ctypes.data))
    return hist


def global_moments_cells(cells, model, tol_q16, exclude=None, window=None):
    """The moments part of the global motion rule on the CPU (bbme_global_moments_host) -> (map (CH, CW) uint8, words (16,)
    int64): model six int32 in Q16, tol_q16 the tolerance in Q16 grid units."""
    cells, exclude, pitch, cw, ch = _gm_grid(cells, exclude, "global_moments_cells")
    model = _gm_model(model, "global_moments_cells")
    gmap = np.empty((ch, cw), np.uint8)
    words = np.empty(16, np.int64)
    _capi.check(_capi.lib().bbme_global_moments_host(cells.ctypes.data, cw, ch, _ptr(exclude), pitch, model.ctypes.data, int(tol_q16),
                                                     _window(window), gmap.ctypes.data, words.ctypes.data))
    return gmap, words


def solve_global_motion(words, kind="affine"):
    """The solve part of the global motion rule (bbme_global_motion_solve_host): sixteen int64 words -> six int32 in Q16."""
    words = np.ascontiguousarray(words, np.int64).reshape(-1)
    if words.size != 16:
        raise _capi.BbmeError(_capi.ERR_INVALID, "solve_global_motion: sixteen int64 words")
    model = np.empty(6, np.int32)
    _capi.check(_capi.lib().bbme_global_motion_solve_host(words.ctypes.data, _gm_kind(kind), model.ctypes.data))
    return model


def global_motion_cells(cells, kind="affine", tol_q16=65536, iterations=3, exclude=None, window=None):
    """The whole estimate of the global motion rule on the CPU (bbme_global_motion_host) -> (model (6,) int32, words (16,)
    int64, map (CH, CW) uint8)."""
    cells, exclude, pitch, cw, ch = _gm_grid(cells, exclude, "global_motion_cells")
    model = np.empty(6, np.int32)
    words = np.empty(16, np.int64)
    gmap = np.empty((ch, cw), np.uint8)
    _capi.check(_capi.lib().bbme_global_motion_host(cells.ctypes.data, cw, ch, _ptr(exclude), pitch, _gm_kind(kind), int(tol_q16),
                                                    int(iterations), _window(window), model.ctypes.data, words.ctypes.data,
                                                    gmap.ctypes.data))
    return model, words, gmap


def global_compensate(image1, image2, model, unit=1, fill=0, window=None):
    """The global compensation rule on the CPU (bbme_global_compensate_host): image1 (None without statistics), image2 uint8
    (H, W) planes (both even), model six int32 in Q16 grid units of 1 / unit pixel -> (compensated plane (H, W) uint8,
    dict(sse, sad, pixels, skipped, mse, psnr) against image1 over window (x0, y0, w, h) in pixels, or None without image1)."""
    image2 = np.ascontiguousarray(image2, np.uint8)
    if image1 is not None:
        image1 = np.ascontiguousarray(image1, np.uint8)
    if image2.ndim != 2 or (image1 is not None and image1.shape != image2.shape):
        raise _capi.BbmeError(_capi.ERR_INVALID, "global_compensate: uint8 planes of one shape (H, W)")
    model = _gm_model(model, "global_compensate")
    h, w = image2.shape
    out = np.empty((h, w), np.uint8)
    s = (C.c_ulonglong * 4)() if image1 is not None else None
    _capi.check(_capi.lib().bbme_global_compensate_host(_ptr(image1), image2.ctypes.data, w, h, model.ctypes.data, int(unit), int(fill),
                                                        _window(window), out.ctypes.data, s))
    return out, (_residual_dict(list(s)) if s is not None else None)


GC_MAX_FRAMES = 32                                        # frames of one cells_global_compensate_bgr_device launch


def global_compensate_bgr(c1, c2, model, unit=1, fill=0, pad_x=0, pad_y=0, window=None):
    """The BGR global compensation rule on the CPU (bbme_global_compensate_bgr_host): c1 (None without statistics), c2 uint8
    (H, W, 3) frames with packed pixels whose rows may be further apart than 3 W bytes (both with the same pitch), model six
    int32 in Q16 grid units of 1 / unit pixel, (pad_x, pad_y) the zero padding of the view the rule works on -> (compensated
    frame (H, W, 3) uint8, dict(sse, sad, pixels, skipped, mse, psnr) against c1 over window (x0, y0, w, h) in frame pixels, or
    None without c1); sse and sad are summed over the three channels, mse = sse / (3 pixels)."""
    def frame(a):
        a = np.asarray(a, np.uint8)
        if a.ndim == 3 and a.shape[2] == 3 and a.strides[2] == 1 and a.strides[1] == 3 and a.strides[0] >= 3 * a.shape[1]:
            return a
        return np.ascontiguousarray(a)

    c2 = frame(c2)
    if c1 is not None:
        c1 = frame(c1)
        if c1.strides[0] != c2.strides[0]:
            c1, c2 = np.ascontiguousarray(c1), np.ascontiguousarray(c2)
    if c2.ndim != 3 or c2.shape[2] != 3 or (c1 is not None and c1.shape != c2.shape):
        raise _capi.BbmeError(_capi.ERR_INVALID, "global_compensate_bgr: uint8 frames of one shape (H, W, 3)")
    model = _gm_model(model, "global_compensate_bgr")
    h, w = c2.shape[:2]
    out = np.empty((h, w, 3), np.uint8)
    s = (C.c_ulonglong * 4)() if c1 is not None else None
    _capi.check(_capi.lib().bbme_global_compensate_bgr_host(_ptr(c1), c2.ctypes.data, w, h, c2.strides[0], int(pad_x), int(pad_y),
                                                            model.ctypes.data, int(unit), int(fill), _window(window), out.ctypes.data,
                                                            3 * w, s))
    return out, (_residual_dict(list(s), 3) if s is not None else None)


def compensate_cells_bgr(c1, c2, grid, unit, fill=0, pad_x=0, pad_y=0, window=None):
    """The BGR compensation rule on the CPU (bbme_compensate_bgr_host): c1 (None without statistics), c2 uint8 (H, W, 3) frames
    with packed pixels whose rows may be further apart than 3 W bytes (both with the same pitch); grid an int16
    ((H + 2 pad_y) / 2, (W + 2 pad_x) / 2, 2) grid of the zero-padded view's cells, whose rows may be further apart, holding
    integer cells (unit=1) or quarter-pel vectors (unit=4) -> (compensated frame (H, W, 3) uint8, dict(sse, sad, pixels, skipped,
    mse, psnr) against c1 over window (x0, y0, w, h) in frame pixels, or None without c1); sse and sad are summed over the three
    channels, mse = sse / (3 pixels)."""
    def frame(a):
        a = np.asarray(a, np.uint8)
        if a.ndim == 3 and a.shape[2] == 3 and a.strides[2] == 1 and a.strides[1] == 3 and a.strides[0] >= 3 * a.shape[1]:
            return a
        return np.ascontiguousarray(a)

    c2 = frame(c2)
    if c1 is not None:
        c1 = frame(c1)
        if c1.strides[0] != c2.strides[0]:
            c1, c2 = np.ascontiguousarray(c1), np.ascontiguousarray(c2)
    if c2.ndim != 3 or c2.shape[2] != 3 or (c1 is not None and c1.shape != c2.shape):
        raise _capi.BbmeError(_capi.ERR_INVALID, "compensate_cells_bgr: uint8 frames of one shape (H, W, 3)")
    h, w = c2.shape[:2]
    grid = np.asarray(grid, np.int16)
    if grid.ndim != 3 or grid.shape[2] != 2:
        raise _capi.BbmeError(_capi.ERR_INVALID, "compensate_cells_bgr: an int16 grid (CH, CW, 2)")
    if not (grid.strides[2] == 2 and grid.strides[1] == 4 and grid.strides[0] >= 4 * grid.shape[1] and grid.strides[0] % 4 == 0):
        grid = np.ascontiguousarray(grid)
    if (2 * grid.shape[0], 2 * grid.shape[1]) != (h + 2 * int(pad_y), w + 2 * int(pad_x)):
        raise _capi.BbmeError(_capi.ERR_INVALID, "compensate_cells_bgr: a grid of %s cells does not cover the %dx%d frame padded by "
                              "(%d, %d)" % (grid.shape[:2], w, h, pad_x, pad_y))
    out = np.empty((h, w, 3), np.uint8)
    s = (C.c_ulonglong * 4)() if c1 is not None else None
    _capi.check(_capi.lib().bbme_compensate_bgr_host(_ptr(c1), c2.ctypes.data, w, h, c2.strides[0], int(pad_x), int(pad_y),
                                                     grid.ctypes.data, grid.strides[0] // 4, int(unit), int(fill), _window(window),
                                                     out.ctypes.data, 3 * w, s))
    return out, (_residual_dict(list(s), 3) if s is not None else None)


def cells_consistency(a, b, tol=1, window=None):
    """The forward-backward consistency rule of include/bbme.h on the CPU (bbme_cells_consistency_host): a, b int16
    (CH, CW, 2) cell grids -> (mask (CH, CW) uint8, dict(consistent, inconsistent, outside, discrepancy) over window
    (cx0, cy0, cw, ch) in cells, None = all cells)."""
    a = np.ascontiguousarray(a, np.int16)
    b = np.ascontiguousarray(b, np.int16)
    if a.ndim != 3 or a.shape[2] != 2 or a.shape != b.shape:
        raise _capi.BbmeError(_capi.ERR_INVALID, "cells_consistency: two int16 grids of one shape (CH, CW, 2)")
    ch, cw = a.shape[:2]
    mask = np.empty((ch, cw), np.uint8)
    s = (C.c_ulonglong * 4)()
    win = _window(window)
    _capi.check(_capi.lib().bbme_cells_consistency_host(a.ctypes.data, b.ctypes.data, cw, ch, int(tol), win, mask.ctypes.data, s))
    return mask, dict(zip(("consistent", "inconsistent", "outside", "discrepancy"), list(s)))


def color_cells(cells, width, height, pad_x=0, pad_y=0, scale=1, maxmotion=-1.0):
    """The colour rule of include/bbme.h on the CPU (bbme_cells_color_host): cells an int16 (CH, CW, 2) grid, the width x height
    frame at (pad_x, pad_y) of its 2 CW x 2 CH plane -> ((ceil(height / scale), ceil(width / scale), 3) uint8 B,G,R,
    (max radius, min u, max u, min v, max v))."""
    cells = np.ascontiguousarray(cells, np.int16)
    if cells.ndim != 3 or cells.shape[2] != 2:
        raise _capi.BbmeError(_capi.ERR_INVALID, "color_cells: an int16 grid of shape (CH, CW, 2)")
    scale = int(scale)
    rows, cols = (-(-int(height) // scale), -(-int(width) // scale)) if scale >= 1 else (0, 0)
    out = np.empty((max(rows, 0), max(cols, 0), 3), np.uint8)
    rng = (C.c_float * 5)()
    _capi.check(_capi.lib().bbme_cells_color_host(cells.ctypes.data, cells.shape[1], cells.shape[0], int(width), int(height),
                                                  int(pad_x), int(pad_y), scale, float(maxmotion), out.ctypes.data, rng))
    return out, tuple(rng)


def _interpolate_cells(what, host, image1, image2, fwd, bwd, num, den, window):
    """interpolate_cells and interpolate_cells_subpel: `host` names the C call, `what` the caller in the errors."""
    image1 = np.ascontiguousarray(image1, np.uint8)
    image2 = np.ascontiguousarray(image2, np.uint8)
    fwd = np.ascontiguousarray(fwd, np.int16)
    bwd = None if bwd is None else np.ascontiguousarray(bwd, np.int16)
    if image1.ndim != 2 or image1.shape != image2.shape:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: two uint8 planes of one shape (H, W)" % what)
    h, w = image1.shape
    if fwd.shape != (h // 2, w // 2, 2) or (bwd is not None and bwd.shape != fwd.shape):
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: int16 grids of shape (H / 2, W / 2, 2)" % what)
    out = np.empty((h, w), np.uint8)
    sel = np.empty((h // 2, w // 2), np.uint8)
    s = (C.c_ulonglong * 4)()
    win = _window(window)
    _capi.check(getattr(_capi.lib(), host)(image1.ctypes.data, image2.ctypes.data, w, h, fwd.ctypes.data,
                                           None if bwd is None else bwd.ctypes.data, int(num), int(den), win,
                                           out.ctypes.data, sel.ctypes.data, s))
    return out, sel, dict(zip(INTERPOLATION_STAT_KEYS, list(s)))


def interpolate_cells(image1, image2, fwd, bwd=None, num=1, den=2, window=None):
    """The interpolation rule of include/bbme.h on the CPU (bbme_interpolate_host): image1, image2 uint8 (H, W) planes of even
    size, fwd and bwd (may be None) int16 (H / 2, W / 2, 2) cell grids -> (frame (H, W) uint8, selection (H / 2, W / 2) uint8,
    dict(forward, backward, zero, cost) over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    return _interpolate_cells("interpolate_cells", "bbme_interpolate_host", image1, image2, fwd, bwd, num, den, window)


def interpolate_cells_subpel(image1, image2, qf, qb=None, num=1, den=2, window=None):
    """The subpel interpolation rule of include/bbme.h on the CPU (bbme_subpel_interpolate_host): interpolate_cells with qf and
    qb (may be None) int16 (H / 2, W / 2, 2) grids of QUARTER-PEL vectors (subpel_cells' output), every cell sampled
    bilinearly at its quarter-pel position -> the same three results."""
    return _interpolate_cells("interpolate_cells_subpel", "bbme_subpel_interpolate_host", image1, image2, qf, qb, num, den, window)


def _temporal_filter_cells(what, cur, prev, next, to_prev, to_next, strength, window, bgr=False, pad_x=0, pad_y=0, subpel=False):
    """temporal_filter_cells (grey planes: they are their own padded view, so no padding and nothing to check about it), with
    subpel temporal_filter_cells_subpel (the same planes, the grids quarter-pel), with bgr temporal_filter_cells_bgr (colour
    frames inside a view padded by pad_x, pad_y) and with both temporal_filter_cells_subpel_bgr; `what` names the caller in the
    errors."""
    shapes = "uint8 frames of one shape (H, W, 3)" if bgr else "uint8 planes of one shape (H, W)"
    grid_shapes = "int16 grids of shape (H0 / 2, W0 / 2, 2)" if bgr else "int16 grids of shape (H / 2, W / 2, 2)"
    cur = np.ascontiguousarray(cur, np.uint8)
    if cur.ndim != (3 if bgr else 2) or (bgr and cur.shape[2] != 3):
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: %s" % (what, shapes))
    h, w = cur.shape[:2]
    pad_x, pad_y = int(pad_x), int(pad_y)
    h0, w0 = h + 2 * pad_y, w + 2 * pad_x                 # the padded view the cells lie on; grey planes are it
    if bgr and (pad_x < 0 or pad_y < 0 or h0 % 2 or w0 % 2):
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: paddings >= 0 that make the padded size even" % what)
    frames, grids = [], []
    for frame, grid in ((prev, to_prev), (next, to_next)):
        frame = None if frame is None else np.ascontiguousarray(frame, np.uint8)
        grid = None if grid is None else np.ascontiguousarray(grid, np.int16)
        if frame is not None and frame.shape != cur.shape:
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: %s" % (what, shapes))
        if grid is not None and grid.shape != (h0 // 2, w0 // 2, 2):
            raise _capi.BbmeError(_capi.ERR_INVALID, "%s: %s" % (what, grid_shapes))
        frames.append(frame)
        grids.append(grid)
    out = np.empty(cur.shape, np.uint8)
    wmap = np.empty((h0 // 2, w0 // 2), np.uint8)
    s = (C.c_ulonglong * 4)()
    size = (w, h, pad_x, pad_y) if bgr else (w, h)
    run = _capi.lib().bbme_temporal_filter_bgr_host if bgr else _capi.lib().bbme_temporal_filter_host
    if subpel:
        run = _capi.lib().bbme_subpel_temporal_filter_bgr_host if bgr else _capi.lib().bbme_subpel_temporal_filter_host
    _capi.check(run(_ptr(frames[0]), cur.ctypes.data, _ptr(frames[1]), *size, _ptr(grids[0]), _ptr(grids[1]), int(strength),
                    _window(window), out.ctypes.data, wmap.ctypes.data, s))
    return out, wmap, dict(zip(TEMPORAL_STAT_KEYS, list(s)))


def temporal_filter_cells(cur, prev=None, next=None, to_prev=None, to_next=None, strength=64, window=None):
    """The temporal filter rule of include/bbme.h on the CPU (bbme_temporal_filter_host): cur, prev, next uint8 (H, W) planes of
    even size, to_prev, to_next int16 (H / 2, W / 2, 2) cell grids on cur; a neighbour is its plane and its grid, either may be
    None -> (frame (H, W) uint8, weights (H / 2, W / 2) uint8 holding wP | wN << 4, dict(prev_cells, next_cells, weight, change)
    over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    return _temporal_filter_cells("temporal_filter_cells", cur, prev, next, to_prev, to_next, strength, window)


def temporal_filter_cells_subpel(cur, prev=None, next=None, q_to_prev=None, q_to_next=None, strength=64, window=None):
    """The subpel temporal filter rule of include/bbme.h on the CPU (bbme_subpel_temporal_filter_host): temporal_filter_cells with
    q_to_prev, q_to_next int16 (H / 2, W / 2, 2) QUARTER-PEL grids on cur (what subpel_cells returns; any int16), each neighbour's
    2x2 cell sampled bilinearly at its quarter-pel position -> the same three results."""
    return _temporal_filter_cells("temporal_filter_cells_subpel", cur, prev, next, q_to_prev, q_to_next, strength, window, subpel=True)


def _grid_rows(grid, shape, what):
    """An int16 (CH, CW, 2) grid as the host rules read it -> (array, row pitch in cells): a view whose cells are packed and whose
    rows lie a whole number of cells apart stays as it is, anything else is copied packed."""
    grid = np.asarray(grid)
    if grid.shape != shape:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: int16 grids of shape %s" % (what, shape))
    if not (grid.dtype == np.int16 and grid.strides[1:] == (4, 2) and grid.strides[0] % 4 == 0 and grid.strides[0] >= 4 * shape[1]):
        grid = np.ascontiguousarray(grid, np.int16)
    return grid, grid.strides[0] // 4


def compose_cells(a, b, unit_shift=0, window=None):
    """The cell composition rule of include/bbme.h on the CPU (bbme_compose_host): a (on frame X into Y) and b (on Y into Z) int16
    (CH, CW, 2) grids, strided row views welcome, unit_shift 0 for pixels or 2 for quarter pels -> (the grid on X into Z
    (CH, CW, 2) int16, dict(clamped, saturated) over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    what = "compose_cells"
    shape = np.shape(a)
    if len(shape) != 3 or shape[2] != 2 or shape[0] < 1 or shape[1] < 1:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: int16 grids of one shape (CH, CW, 2)" % what)
    a, pa = _grid_rows(a, shape, what)
    b, pb = _grid_rows(b, shape, what)
    out = np.empty(shape, np.int16)
    s = (C.c_ulonglong * 2)()
    _capi.check(_capi.lib().bbme_compose_host(a.ctypes.data, pa, b.ctypes.data, pb, shape[1], shape[0], int(unit_shift), _window(window),
                                              out.ctypes.data, shape[1], s))
    return out, dict(zip(COMPOSE_STAT_KEYS, list(s)))


def temporal_filter_cells_wide(cur, planes, grids, strength=64, window=None):
    """The wide temporal filter rule of include/bbme.h on the CPU (bbme_wide_temporal_filter_host): cur a uint8 (H, W) plane of even
    size; planes and grids sequences of four, P1, N1, P2, N2, None = absent: uint8 (H, W) planes and int16 (H / 2, W / 2, 2)
    QUARTER-PEL grids on cur (strided row views of one common pitch stay as they are) -> (frame (H, W) uint8, weights
    (H / 2, W / 2) uint16 holding w_k << 4 k, dict(prev1_cells, next1_cells, prev2_cells, next2_cells, weight, change) over
    window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    what = "temporal_filter_cells_wide"
    cur = np.ascontiguousarray(cur, np.uint8)
    planes, grids = list(planes), list(grids)
    if cur.ndim != 2 or len(planes) != 4 or len(grids) != 4:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: a uint8 (H, W) plane, four planes and four grids (None = absent)" % what)
    h, w = cur.shape
    planes = [None if p is None else np.ascontiguousarray(p, np.uint8) for p in planes]
    if any(p is not None and p.shape != cur.shape for p in planes):
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: uint8 planes of one shape (H, W)" % what)
    rows = [None if g is None else _grid_rows(g, (h // 2, w // 2, 2), what) for g in grids]
    if len({r[1] for r in rows if r is not None}) > 1:                 # no common pitch: packed copies have one
        rows = [None if r is None else (np.ascontiguousarray(r[0]), w // 2) for r in rows]
    grids = [None if r is None else r[0] for r in rows]
    pitch = next((r[1] for r in rows if r is not None), w // 2)
    out = np.empty(cur.shape, np.uint8)
    wmap = np.empty((h // 2, w // 2), np.uint16)
    s = (C.c_ulonglong * 6)()
    _capi.check(_capi.lib().bbme_wide_temporal_filter_host(_ptr4(planes), cur.ctypes.data, w, h, _ptr4(grids), pitch, int(strength),
                                                           _window(window), out.ctypes.data, wmap.ctypes.data, s))
    return out, wmap, dict(zip(WIDE_STAT_KEYS, list(s)))


def temporal_filter_cells_wide_bgr(cur, frames, grids, strength=64, pad_x=0, pad_y=0, window=None):
    """The BGR wide temporal filter rule of include/bbme.h on the CPU (bbme_wide_temporal_filter_bgr_host): cur a uint8 (H, W, 3)
    colour frame, read as if zero-padded by (pad_x, pad_y) to an even H0 x W0; frames and grids sequences of four, P1, N1, P2, N2,
    None = absent: uint8 (H, W, 3) frames and int16 (H0 / 2, W0 / 2, 2) QUARTER-PEL grids on cur (strided row views of one common
    pitch stay as they are) -> (frame (H, W, 3) uint8, weights (H0 / 2, W0 / 2) uint16 holding w_k << 4 k, dict(prev1_cells,
    next1_cells, prev2_cells, next2_cells, weight, change) over window (cx0, cy0, cw, ch) in cells, None = all cells)."""
    what = "temporal_filter_cells_wide_bgr"
    cur = np.ascontiguousarray(cur, np.uint8)
    frames, grids = list(frames), list(grids)
    if cur.ndim != 3 or cur.shape[2] != 3 or len(frames) != 4 or len(grids) != 4:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: a uint8 (H, W, 3) frame, four frames and four grids (None = absent)" % what)
    h, w = cur.shape[:2]
    pad_x, pad_y = int(pad_x), int(pad_y)
    frames = [None if p is None else np.ascontiguousarray(p, np.uint8) for p in frames]
    if any(p is not None and p.shape != cur.shape for p in frames):
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: uint8 frames of one shape (H, W, 3)" % what)
    if pad_x < 0 or pad_y < 0 or (w + 2 * pad_x) % 2 or (h + 2 * pad_y) % 2:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: paddings (%d, %d) do not give an even padded view" % (what, pad_x, pad_y))
    ch, cw = (h + 2 * pad_y) // 2, (w + 2 * pad_x) // 2
    rows = [None if g is None else _grid_rows(g, (ch, cw, 2), what) for g in grids]
    if len({r[1] for r in rows if r is not None}) > 1:                 # no common pitch: packed copies have one
        rows = [None if r is None else (np.ascontiguousarray(r[0]), cw) for r in rows]
    grids = [None if r is None else r[0] for r in rows]
    pitch = next((r[1] for r in rows if r is not None), cw)
    out = np.empty(cur.shape, np.uint8)
    wmap = np.empty((ch, cw), np.uint16)
    s = (C.c_ulonglong * 6)()
    _capi.check(_capi.lib().bbme_wide_temporal_filter_bgr_host(_ptr4(frames), cur.ctypes.data, w, h, pad_x, pad_y, _ptr4(grids), pitch,
                                                               int(strength), _window(window), out.ctypes.data, wmap.ctypes.data, s))
    return out, wmap, dict(zip(WIDE_STAT_KEYS, list(s)))


def temporal_filter_cells_bgr(cur, prev=None, next=None, to_prev=None, to_next=None, strength=64, pad_x=0, pad_y=0, window=None):
    """The BGR temporal filter rule of include/bbme.h on the CPU (bbme_temporal_filter_bgr_host): cur, prev, next uint8 (H, W, 3)
    colour frames, read as if zero-padded by (pad_x, pad_y) to an even H0 x W0, to_prev, to_next int16 (H0 / 2, W0 / 2, 2) cell
    grids on cur; a neighbour is its frame and its grid, either may be None -> (frame (H, W, 3) uint8, weights (H0 / 2, W0 / 2)
    uint8 holding wP | wN << 4, dict(prev_cells, next_cells, weight, change) over window (cx0, cy0, cw, ch) in cells, None = all
    cells)."""
    return _temporal_filter_cells("temporal_filter_cells_bgr", cur, prev, next, to_prev, to_next, strength, window, bgr=True,
                                  pad_x=pad_x, pad_y=pad_y)


def temporal_filter_cells_subpel_bgr(cur, prev=None, next=None, q_to_prev=None, q_to_next=None, strength=64, pad_x=0, pad_y=0,
                                     window=None):
    """The BGR subpel temporal filter rule of include/bbme.h on the CPU (bbme_subpel_temporal_filter_bgr_host):
    temporal_filter_cells_bgr with q_to_prev, q_to_next int16 (H0 / 2, W0 / 2, 2) QUARTER-PEL grids on cur (what subpel_cells returns
    on the padded luma planes; any int16), each neighbour's 2x2 cell sampled bilinearly at its quarter-pel position of the
    zero-padded view -> the same three results."""
    return _temporal_filter_cells("temporal_filter_cells_subpel_bgr", cur, prev, next, q_to_prev, q_to_next, strength, window, bgr=True,
                                  pad_x=pad_x, pad_y=pad_y, subpel=True)


def bgr_to_gray(frame):
    """The luma rule of include/bbme.h on the CPU (bbme_bgr_to_gray_host): frame uint8 (H, W, 3) in B,G,R order, its rows any
    distance >= 3 W apart (a column slice of a wider array is read in place) -> (H, W) uint8,
    Y = (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise _capi.BbmeError(_capi.ERR_INVALID, "bgr_to_gray: a uint8 frame of shape (H, W, 3)")
    h, w = frame.shape[:2]
    if frame.strides[1:] != (3, 1) or frame.strides[0] < 3 * w:
        frame = np.ascontiguousarray(frame)
    out = np.empty((h, w), np.uint8)
    _capi.check(_capi.lib().bbme_bgr_to_gray_host(frame.ctypes.data, w, h, frame.strides[0], out.ctypes.data))
    return out


def _interpolate_cells_bgr(what, host, luma1, luma2, bgr1, bgr2, fwd, bwd, num, den, pad_x, pad_y):
    """interpolate_cells_bgr and interpolate_cells_subpel_bgr: `host` names the C call, `what` the caller in the errors."""
    luma1 = np.ascontiguousarray(luma1, np.uint8)
    luma2 = np.ascontiguousarray(luma2, np.uint8)
    bgr1 = np.ascontiguousarray(bgr1, np.uint8)
    bgr2 = np.ascontiguousarray(bgr2, np.uint8)
    fwd = np.ascontiguousarray(fwd, np.int16)
    bwd = None if bwd is None else np.ascontiguousarray(bwd, np.int16)
    if luma1.ndim != 2 or luma1.shape != luma2.shape or bgr1.ndim != 3 or bgr1.shape[2] != 3 or bgr1.shape != bgr2.shape:
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: two uint8 planes (H0, W0) and two uint8 frames (H, W, 3)" % what)
    h0, w0 = luma1.shape
    h, w = bgr1.shape[:2]
    if fwd.shape != (h0 // 2, w0 // 2, 2) or (bwd is not None and bwd.shape != fwd.shape):
        raise _capi.BbmeError(_capi.ERR_INVALID, "%s: int16 grids of shape (H0 / 2, W0 / 2, 2)" % what)
    out = np.empty((h, w, 3), np.uint8)
    _capi.check(getattr(_capi.lib(), host)(luma1.ctypes.data, luma2.ctypes.data, w0, h0, bgr1.ctypes.data, bgr2.ctypes.data,
                                           w, h, int(pad_x), int(pad_y), fwd.ctypes.data,
                                           None if bwd is None else bwd.ctypes.data, int(num), int(den), out.ctypes.data))
    return out


def interpolate_cells_bgr(luma1, luma2, bgr1, bgr2, fwd, bwd=None, num=1, den=2, pad_x=0, pad_y=0):
    """The BGR interpolation rule of include/bbme.h on the CPU (bbme_interpolate_bgr_host): luma1, luma2 the padded uint8
    (H0, W0) luma planes, bgr1, bgr2 the uint8 (H, W, 3) colour frames whose lumas they hold at (pad_x, pad_y) (H0 = H + 2 pad_y,
    W0 = W + 2 pad_x), fwd and bwd (may be None) int16 (H0 / 2, W0 / 2, 2) cell grids -> the unpadded (H, W, 3) uint8 frame."""
    return _interpolate_cells_bgr("interpolate_cells_bgr", "bbme_interpolate_bgr_host", luma1, luma2, bgr1, bgr2, fwd, bwd, num, den,
                                  pad_x, pad_y)


def interpolate_cells_subpel_bgr(luma1, luma2, bgr1, bgr2, qf, qb=None, num=1, den=2, pad_x=0, pad_y=0):
    """The BGR subpel interpolation rule of include/bbme.h on the CPU (bbme_subpel_interpolate_bgr_host): interpolate_cells_bgr
    with qf and qb (may be None) int16 (H0 / 2, W0 / 2, 2) grids of QUARTER-PEL vectors (subpel_cells' output), every pixel of
    both colour frames sampled bilinearly at its quarter-pel position -> the unpadded (H, W, 3) uint8 frame."""
    return _interpolate_cells_bgr("interpolate_cells_subpel_bgr", "bbme_subpel_interpolate_bgr_host", luma1, luma2, bgr1, bgr2, qf, qb,
                                  num, den, pad_x, pad_y)


def plan_padding(width, height, search_size, block_size):
    """padded_width, padded_height, padding_x, padding_y of MF::MF (motion_framework.cpp:14-54)."""
    p = _capi.make_params(search_size, block_size)
    v = [C.c_int() for _ in range(4)]
    _capi.check(_capi.lib().bbme_plan_padding(width, height, C.byref(p), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def pad_zero(img, pad_x, pad_y):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.empty((h + 2 * pad_y, w + 2 * pad_x), np.uint8)
    _capi.check(_capi.lib().bbme_pad_zero_host(img.ctypes.data, w, h, w, pad_x, pad_y, out.ctypes.data))
    return out


def pyr_down(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.empty((h // 2, w // 2), np.uint8)
    _capi.check(_capi.lib().bbme_pyr_down_host(img.ctypes.data, w, h, out.ctypes.data))
    return out


def resize_x4(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.empty((h * 4, w * 4), np.uint8)
    _capi.check(_capi.lib().bbme_resize_x4_host(img.ctypes.data, w, h, out.ctypes.data))
    return out
