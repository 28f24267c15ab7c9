"""Frame pairs of a sequence over GPUs and within one GPU.

Pairs are independent in the reference (an MF object holds all state of one pair,
motion_framework.h:37-46; nothing is carried from pair to pair), so they shard with no exchange:

* across GPUs -- pair p goes to rank p % world_size (one process per GPU) and runs the whole pyramid there; the only
  collective is ONE gather per step of the results on rank 0.  `CellGather` / `mf_cell_gather` is that step as
  `bench.py --gpus N` runs it: the results travel as compact int16 cell grids (1/16 of the dense field), staging buffers are
  double-buffered, and rank 0 expands the gathered grids to the dense .flo fields on a second stream beside the next
  estimate.  (`csrc/seq_schedule.hpp` + `bbme_seq` is the same pipeline in C++ over RCCL, without torch.)
* within a GPU -- `estimate_pairs_pipelined`: the pairs that share a GPU go into BATCHED contexts (`MFBatch`,
  bbme_create_batch: every kernel works on all pairs of a context at once), a few contexts side by side on their own streams.
* a video -- frames f0, f1, ... whose pairs (f0, f1), (f1, f2), ... share every inner frame: `estimate_frames_pipelined` on
  chain contexts (`MFChain`, bbme_create_chain), dealt in contiguous segments (`plan_frame_segments`, `shard_frames`), sets
  every frame once where the pair form sets it twice.
* `estimate_sequence` is the convenience form on top of any `compute` callable and any torch.distributed backend ("nccl" is
  RCCL over xGMI on ROCm; "gloo" in the CPU tests): it gathers the finished dense fields round by round and optionally writes
  the .flo files.  It is not the timed path.
"""
import os

import numpy as np

from . import _capi


def local_device():
    """The GPU of this process: one process per GPU, LOCAL_RANK as torch.distributed.run exports it."""
    return int(os.environ.get("LOCAL_RANK", "0"))


def cells_to_words(cells):
    """(rows, cols, 2) int16 (dx, dy) per 2x2 cell -> (rows, cols) int32 words, dx in the low half: the layout of the
    MV grids in HBM and the unit the gather moves (NCCL has no int16)."""
    c = np.ascontiguousarray(cells, np.int16)
    return c.view(np.int32).reshape(c.shape[0], c.shape[1])


def flow_to_cells(flow_padded):
    """The dense padded field -> its 2x2-cell grid (the field is constant on 2x2 cells, motion_framework.cpp:205-206)."""
    return np.ascontiguousarray(flow_padded[::2, ::2]).astype(np.int16)


def expand_cells_host(words):
    """copy_to_all_pixels (motion_framework.cpp:815-826) on the host: (rows, cols) int32 words -> dense
    (2*rows, 2*cols, 2) float32.  The CPU stand-in for bbme_expand_cells_device in the gloo tests."""
    w = np.ascontiguousarray(words, np.int32)
    mv = w.view(np.int16).reshape(w.shape[0], w.shape[1], 2).astype(np.float32)
    return np.repeat(np.repeat(mv, 2, axis=0), 2, axis=1)


class CellGather:
    """The multi-GPU step of a sequence (BASELINE configs[4]): every rank estimates one pair per step, the
    results travel as compact cell grids -- one packed int16 (dx, dy) pair per 2x2 cell, 16x smaller than the dense
    field and exactly the same information -- in ONE gather to rank 0 (torch.distributed: "nccl" is RCCL over xGMI;
    "gloo" in the CPU tests), and rank 0 expands every gathered grid to the dense .flo field.

    estimate()                 enqueues this rank's estimate (GPU: on the current stream, no host wait; CPU: computes)
    cells                      torch int32 tensor (rows, cols) the estimate leaves its result in
    expand(words, flow, strm)  rank 0: one gathered grid -> dense (2*rows, 2*cols, 2) float32 tensor `flow`;
                               strm = raw HIP stream handle the expansion must run on (None on the CPU)
    On a GPU, with `overlap` (default), the gather of step i and rank 0's expansions run on a second stream beside the
    estimate of step i + 1: each step copies its grid into one of two staging buffers; events order the two streams.
    With overlap=False the estimate, the gather and the expansions are simply enqueued in order on the work stream.  That is
    the better form when the estimate is a hipGraph with a forked branch (the speculative search): a second stream waiting
    for an event recorded behind such a graph costs the next replay about 0.7 ms on ROCm 7 (scripts/dist_step_probe.py:
    1.75 -> 2.45 ms per 4K step), far more than the ~0.1 ms of gather and expansions it would hide.  bench.py measures
    both pairings before the timed region and keeps the faster.  `flows` (rank 0) holds the dense fields of the last
    finished step, one per rank.
    """

    def __init__(self, estimate, cells, expand, group=None, dst=0, overlap=True):
        import torch
        import torch.distributed as dist
        self._dist, self._torch = dist, torch
        self.estimate, self.cells, self.expand = estimate, cells, expand
        self.group, self.dst, self.overlap = group, dst, overlap
        self.rank = dist.get_rank(group)
        self.world = dist.get_world_size(group)
        self.on_gpu = cells.is_cuda
        rows, cols = cells.shape
        root = self.rank == dst
        self.gather_list = [torch.empty_like(cells) for _ in range(self.world)] if root else None
        self.flows = torch.empty((self.world, 2 * rows, 2 * cols, 2), dtype=torch.float32, device=cells.device) if root else None
        self.stage = [torch.empty_like(cells) for _ in range(2)]
        self.steps = 0
        if self.on_gpu:
            self.work_stream = torch.cuda.current_stream(cells.device)
            self.side_stream = torch.cuda.Stream(device=cells.device)
            self.ev_ready = [torch.cuda.Event() for _ in range(2)]
            self.ev_free = [torch.cuda.Event() for _ in range(2)]

    def step(self):
        dist, torch = self._dist, self._torch
        b = self.steps & 1
        self.steps += 1
        if not self.on_gpu:
            self.estimate()
            self.stage[b].copy_(self.cells)
            dist.gather(self.stage[b], self.gather_list, dst=self.dst, group=self.group)
            if self.rank == self.dst:
                for r in range(self.world):
                    self.expand(self.gather_list[r], self.flows[r], None)
            return
        if not self.overlap:
            self.estimate()
            with torch.cuda.stream(self.work_stream):
                dist.gather(self.cells, self.gather_list, dst=self.dst, group=self.group)
                if self.rank == self.dst:
                    for r in range(self.world):
                        self.expand(self.gather_list[r], self.flows[r], self.work_stream.cuda_stream)
            return
        self.work_stream.wait_event(self.ev_free[b])      # the gather that read this staging buffer two steps ago is done
        self.estimate()
        with torch.cuda.stream(self.work_stream):
            self.stage[b].copy_(self.cells)
        self.ev_ready[b].record(self.work_stream)
        with torch.cuda.stream(self.side_stream):
            self.side_stream.wait_event(self.ev_ready[b])
            dist.gather(self.stage[b], self.gather_list, dst=self.dst, group=self.group)
            if self.rank == self.dst:
                for r in range(self.world):
                    self.expand(self.gather_list[r], self.flows[r], self.side_stream.cuda_stream)
            self.ev_free[b].record(self.side_stream)

    def fence(self):
        """Both streams idle on every rank."""
        if self.on_gpu:
            self.side_stream.synchronize()
            self.work_stream.synchronize()
        self._dist.barrier(group=self.group)


def mf_cell_gather(mf, device, group=None, overlap=True):
    """CellGather over a context (MF) whose frames are set: the estimate, the context's cell grid and
    bbme_expand_cells_device_on.  The context is moved onto torch's current stream, which must not be the default
    stream (handle 0 means "private stream" to bbme_set_stream)."""
    import torch
    stream = torch.cuda.current_stream(device)
    if stream.cuda_stream == 0:
        raise ValueError("mf_cell_gather: run under an explicit torch.cuda.Stream (the default stream has handle 0)")
    mf.set_stream(stream.cuda_stream)

    class _View:
        pass
    v = _View()
    v.__cuda_array_interface__ = {"shape": (mf.padded_height // 2, mf.padded_width // 2), "typestr": "<i4",
                                  "data": (mf.cells_device_ptr(), False), "version": 2, "strides": None}
    cells = torch.as_tensor(v, device=torch.device("cuda", device))

    def expand(words, flow, strm):
        mf.expand_cells_device(words.data_ptr(), flow.data_ptr(), strm)
    return CellGather(mf.estimate_async, cells, expand, group=group, overlap=overlap)


def shard_pairs(n_pairs, rank, world_size):
    """Global indices of the pairs rank `rank` computes."""
    return list(range(rank, n_pairs, world_size))


def estimate_pairs_pipelined(pairs, search_size, block_size, device=None, in_flight=4, batch=2):
    """All pairs of `pairs` (a list of (frame1, frame2), equal sizes) on ONE GPU, `in_flight` of them at a time.

    The pairs go, `batch` at a time, into batched contexts (MFBatch: one launch sequence for all pairs of the context, the
    pair is a grid dimension), in_flight // batch contexts created once (level state, launch graph) and re-used round-robin,
    each on its own stream: while one context's regulariser walks its dependency chains the chip searches for another.
    Why batches: the device dispatches the dependent kernels of many streams no faster than one per ~4 us chip-wide, so one
    context per pair is dispatch-bound at 69 launches per pair (8 pairs at 4K: 34 Mblocks/s with 8 contexts x 1 pair,
    45 with 4 x 2).  Returns the unpadded (H, W, 2) float32 fields in input order; a pair's result does not depend on
    what shares its context or the GPU (tests/test_gpu_parity.py).  More than 4 streams: export GPU_MAX_HW_QUEUES (e.g. 16)
    before the process starts the HIP runtime.
    """
    from .motion_framework import MFBatch
    if not pairs:
        return []
    if device is None:
        device = local_device()
    per = max(1, min(batch, in_flight, len(pairs)))
    n_slots = max(1, in_flight // per)
    groups = [list(range(i, min(i + per, len(pairs)))) for i in range(0, len(pairs), per)]
    slots = []
    out = [None] * len(pairs)
    pending = []                                           # (slot, pair indices), oldest first

    def collect():
        slot, idxs = pending.pop(0)
        mf = slots[slot]
        for p, idx in enumerate(idxs):
            h, w = pairs[idx][0].shape
            flow = mf.get_pair_flow(p)                     # waits for this context's stream only
            out[idx] = np.ascontiguousarray(flow[mf.padding_y:mf.padding_y + h, mf.padding_x:mf.padding_x + w])

    try:
        for idxs in groups:
            frames = [pairs[i] for i in idxs] + [pairs[idxs[-1]]] * (per - len(idxs))     # a short last group: padded, not read
            if len(slots) < n_slots:
                slots.append(MFBatch(frames, search_size, block_size, len(block_size), device=device))
                slot = len(slots) - 1
                if n_slots * per > 1:
                    slots[slot].set_speculation(False)      # the other pairs in flight fill the chip already
            else:
                slot = pending[0][0]
                collect()
                for p, (f1, f2) in enumerate(frames):
                    slots[slot].set_pair(p, f1, f2)
            slots[slot].estimate_async()
            pending.append((slot, idxs))
        while pending:
            collect()
    finally:
        for mf in slots:
            mf.close()
    return out


def plan_frame_segments(n_pairs, slots, batch):
    """The rounds, in issue order, of the `n_pairs` consecutive pairs of a video (pair p = frames p, p + 1) on `slots` chain
    contexts (MFChain) of at most `batch` pairs: [(slot, first_pair, count, carry), ...].

    The pairs are cut into `slots` CONTIGUOUS segments whose lengths differ by at most one (empty ones dropped), one per
    context, and every context walks its segment `batch` pairs a round; rounds are issued round-robin over the contexts.
    `carry` is true when the context's previous round ended at first_pair: frame first_pair is then already on the GPU (its
    last slot, rolled to slot 0 by MFChain.advance) and the round sets `count` frames; a context's first round sets count + 1.
    So the frames set in total are n_pairs + (number of segments) against 2 * n_pairs for independent pairs.
    Dealing the PAIRS round-robin, as estimate_pairs_pipelined does, would hand a context frames 0..2, then 8..10: nothing to
    carry.  Contiguous segments are what make the roll pay, and they are also how the frames of a video have to be dealt to
    GPUs (shard_frames)."""
    if n_pairs < 0 or slots < 1 or batch < 1:
        raise ValueError("plan_frame_segments: n_pairs >= 0, slots >= 1 and batch >= 1")
    base, extra = divmod(n_pairs, slots)
    segments, start = [], 0
    for s in range(slots):
        n = base + (1 if s < extra else 0)
        if n:
            segments.append((start, start + n))
        start += n
    rounds, done = [], [seg[0] for seg in segments]
    while any(done[s] < segments[s][1] for s in range(len(segments))):
        for s, (lo, hi) in enumerate(segments):
            if done[s] < hi:
                count = min(batch, hi - done[s])
                rounds.append((s, done[s], count, done[s] != lo))
                done[s] += count
    return rounds


def shard_frames(n_frames, rank, world_size):
    """(first_frame, last_frame) of the contiguous run of a video's frames rank `rank` takes -- it computes the pairs
    first_frame .. last_frame - 1 -- or None when it takes none.  The video counterpart of shard_pairs: the n_frames - 1 pairs
    in `world_size` contiguous segments (plan_frame_segments with one round per rank), so that ranks share only their boundary
    frames; shard_pairs' round-robin would give every rank both frames of every pair it owns."""
    n_pairs = max(n_frames - 1, 0)
    base, extra = divmod(n_pairs, world_size)
    first = rank * base + min(rank, extra)
    count = base + (1 if rank < extra else 0)
    return (first, first + count) if count else None


def _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect, bidirectional=False, upsample=1):
    """The loop of every video driver: the len(frames) - 1 consecutive pairs on chain contexts (MFChain) that follow
    plan_frame_segments -- in_flight // batch contexts, each walking a contiguous segment of the video.  A context's first
    round sets count + 1 frames, every later round rolls its last frame to slot 0 (MFChain.advance) and sets `count`; a short
    round is padded by repeating its last frame (the padded pairs are not read).  Every round enqueues estimate_async, or
    estimate_bidirectional_async with `bidirectional`, and collect(mf, first, count) reads the products of its pairs
    first .. first + count - 1 from the context's pairs 0 .. count - 1 (a read waits for that context's stream only).
    COLLECT BEFORE ADVANCE: the roll and the next estimate overwrite the planes and grids that collect reads, so a round is
    collected before its context advances, and the rounds still in flight at the end in slot order.  Speculation is switched
    off when several pairs are in flight (they fill the chip already); every context is closed, also when a read raises."""
    from .motion_framework import MFChain
    n_pairs = len(frames) - 1
    per = max(1, min(batch, in_flight, n_pairs))
    n_slots = max(1, in_flight // per)
    rounds = plan_frame_segments(n_pairs, n_slots, per)
    n_ctx = 1 + max(r[0] for r in rounds)
    chains = [None] * n_ctx
    pending = [None] * n_ctx                               # per context: (first_pair, count) of the round in flight

    def drain(slot):
        first, count = pending[slot]
        pending[slot] = None
        collect(chains[slot], first, count)

    try:
        for slot, first, count, carry in rounds:
            run = frames[first + 1:first + count + 1]
            run = run + [run[-1]] * (per - count)
            if not carry:
                chains[slot] = MFChain([frames[first]] + run, search_size, block_size, len(block_size), device=device,
                                       upsample=upsample)
                if n_ctx * per > 1:
                    chains[slot].set_speculation(False)
            else:
                drain(slot)
                chains[slot].advance(run)
            if bidirectional:
                chains[slot].estimate_bidirectional_async()
            else:
                chains[slot].estimate_async()
            pending[slot] = (first, count)
        for slot in range(n_ctx):
            if pending[slot]:
                drain(slot)
    finally:
        for mf in chains:
            if mf is not None:
                mf.close()


def estimate_frames_pipelined(frames, search_size, block_size, device=None, in_flight=4, batch=2, upsample=1, subpel=False):
    """The len(frames) - 1 consecutive pairs of a video on ONE GPU: the unpadded (H, W, 2) float32 fields in order, the same
    as estimate_pairs_pipelined(list(zip(frames, frames[1:])), ...), but on chain contexts (MFChain) that follow
    plan_frame_segments: in_flight // batch contexts, each walking a contiguous segment of the video; a context's first round
    sets count + 1 frames, every later round rolls its last frame to slot 0 and sets `count`.  A short last round is padded by
    repeating its last frame (the padded pairs are not read).  upsample=4: original frames, fields of the up-sampled size.
    subpel=True: instead of the fields, every pair's cells refined to quarter-pel on its level-0 planes (MF.subpel_cells), the
    padded (CH, CW, 2) int16 grids in quarter pixels (of the up-sampled frame with upsample=4)."""
    frames = list(frames)
    n_pairs = len(frames) - 1
    if n_pairs < 1:
        return []
    if device is None:
        device = local_device()
    out = [None] * n_pairs

    def collect(mf, first, count):
        h, w = mf.orig_height, mf.orig_width
        for p in range(count):
            if subpel:
                out[first + p] = mf.get_pair_subpel_cells(p)       # waits for this context's stream only
                continue
            flow = mf.get_pair_flow(p)                     # waits for this context's stream only
            out[first + p] = np.ascontiguousarray(flow[mf.padding_y:mf.padding_y + h, mf.padding_x:mf.padding_x + w])

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect, upsample=upsample)
    return out


def estimate_frames_bidirectional(frames, search_size, block_size, device=None, in_flight=4, batch=2, upsample=1, tol=1):
    """Both fields of the len(frames) - 1 consecutive pairs of a video on ONE GPU, and their forward-backward consistency, on
    the chain plan of estimate_frames_pipelined (same contexts, rounds and padding of a short round): every frame is still
    set once, and MFChain.estimate_bidirectional_async estimates pair p = (f_p, f_p+1) and (f_p+1, f_p) from the same planes.
    Returns one tuple per pair: (forward (H, W, 2) float32, backward (H, W, 2) float32 -- the unpadded fields, the backward
    one expanded on the host from its cells --, forward mask, backward mask -- uint8 consistency classes at tolerance `tol`
    over the cells whose top-left pixel lies in the unpadded frame, MF.default_cell_window)."""
    frames = list(frames)
    n_pairs = len(frames) - 1
    if n_pairs < 1:
        return []
    if device is None:
        device = local_device()
    out = [None] * n_pairs

    def collect(mf, first, count):
        h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
        cx0, cy0, cw, ch = mf.default_cell_window()
        for p in range(count):
            fwd = mf.get_pair_flow(p)                      # waits for this context's stream only
            bwd = expand_cells_host(mf.get_pair_backward_cells(p).view(np.int32)[..., 0])
            masks = [mf.consistency(which, tol, pair=p)[cy0:cy0 + ch, cx0:cx0 + cw].copy() for which in ("forward", "backward")]
            out[first + p] = (np.ascontiguousarray(fwd[py:py + h, px:px + w]), np.ascontiguousarray(bwd[py:py + h, px:px + w]),
                              masks[0], masks[1])

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect, bidirectional=True, upsample=upsample)
    return out


def interpolate_frames(frames, search_size, block_size, factor, device=None, in_flight=4, batch=2, subpel_bgr=False, subpel=False):
    """Frame-rate up-conversion of a video on ONE GPU: every original frame, and factor - 1 interpolated frames (phases k /
    factor, the interpolation rule of include/bbme.h) between each consecutive two -> factor * (len(frames) - 1) + 1 uint8
    (H, W) frames, the interpolated ones the unpadded windows of the padded result.  Runs on the chain plan of
    estimate_frames_bidirectional (same contexts, rounds and padding of a short round): every frame is set once, both fields
    of a pair come from the same planes, and the factor - 1 frames of a pair from one launch (MF.interpolate_run).
    Colour video: (H, W, 3) frames in B,G,R order give (H, W, 3) frames on the same plan -- the luma planes are made on the
    GPU from the colour frames (the luma rule), the fields are the luma's, and the frames in between come from the stored
    colour by the BGR interpolation rule (MF.interpolate_run_bgr); still every frame is set once.
    subpel=True: the frames in between come from the subpel interpolation rule on the same plan (MF.interpolate_run_subpel:
    both fields refined to quarter-pel, the cells placed and sampled at quarter-pel positions).  Grey video only: colour frames
    with subpel=True are a ValueError.
    subpel_bgr=True is the way to get quarter-pel colour: the colour frames in between come from the BGR subpel interpolation
    rule on the same plan (MF.interpolate_run_subpel_bgr: the quarter-pel selection on the luma planes, both stored colour frames
    sampled bilinearly at the quarter-pel positions); still every frame is set once.  Colour video only: grey frames with
    subpel_bgr=True are a ValueError."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    bgr = bool(frames) and frames[0].ndim == 3
    factor = int(factor)
    if not 2 <= factor <= 256:
        raise ValueError("interpolate_frames: factor %d outside 2..256" % factor)
    if bgr and subpel:
        raise ValueError("interpolate_frames: subpel=True takes grey frames; colour output keeps the integer rule")
    if subpel_bgr and frames and not bgr:
        raise ValueError("interpolate_frames: subpel_bgr=True takes colour frames (H, W, 3); grey frames take subpel=True")
    n_pairs = len(frames) - 1
    if n_pairs < 1:
        return frames
    if device is None:
        device = local_device()
    between = [None] * n_pairs

    def collect(mf, first, count):
        h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
        for p in range(count):
            if bgr:
                between[first + p] = list(mf.interpolate_run_subpel_bgr(factor, pair=p) if subpel_bgr
                                          else mf.interpolate_run_bgr(factor, pair=p))
                continue
            run = mf.interpolate_run_subpel(factor, pair=p) if subpel else mf.interpolate_run(factor, pair=p)      # waits for this context's stream only
            between[first + p] = [np.ascontiguousarray(f[py:py + h, px:px + w]) for f in run]

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect, bidirectional=True)
    out = []
    for p in range(n_pairs):
        out.append(frames[p])
        out.extend(between[p])
    out.append(frames[-1])
    return out


def denoise_frames(frames, search_size, block_size, strength, device=None, in_flight=4, batch=2, subpel=False, subpel_bgr=False):
    """Motion-compensated temporal denoising of a video on ONE GPU (the temporal filter rule of include/bbme.h): every
    frame averaged with its two motion-aligned neighbours wherever their 2x2 cells match better than `strength` -> len(frames)
    unpadded uint8 (H, W) frames.  A COLOUR video, (H, W, 3) frames in B,G,R order, gives (H, W, 3) frames by the BGR temporal
    filter rule: the motion is estimated on the luma and the weights come from the colour frames (this function used to promise
    grey frames only; what it did with colour ones was never defined).  The first and the last frame of the video have one
    neighbour, every other frame two, the frames at round and segment boundaries included.  Runs on the chain plan of estimate_frames_bidirectional (same contexts,
    rounds and padding of a short round): every frame is set once and every pair estimated once, both ways.  A round's inner
    frames come from one launch (MFChain.temporal_filter_run).  A frame at a boundary -- the last of one round and the first
    of the next, of the same context (carried by advance) or of the neighbouring one -- has its previous frame and the grid
    into it in one round and its next frame and the grid into that in the other: the round that comes first copies its half on
    the GPU (planes and grid; the roll and the next estimate overwrite them) and the other filters the frame through
    MF.cells_temporal_filter_device from the copies and its own buffers.  No plane or grid goes through the host.  In colour
    the same plan, rounds and copies, of the stored colour frames in the planes' place (MFChain.temporal_filter_run_bgr,
    MF.frame_bgr_tensor, MF.cells_temporal_filter_bgr_device).
    With subpel (grey video only) the SUBPEL TEMPORAL FILTER RULE: the same plan, every grid refined to quarter pels before it is
    used (MFChain.temporal_filter_run_subpel; at a boundary MF.cells_subpel_device makes the copy of a grid, so the copies hold
    quarter-pel grids, and MF.cells_temporal_filter_subpel_device filters).  A colour video with subpel is BbmeError
    (ERR_UNSUPPORTED): the BGR temporal filter rule is integer.
    With subpel_bgr (colour video only; grey frames are a ValueError) the BGR SUBPEL TEMPORAL FILTER RULE: the colour plan, every
    grid refined to quarter pels on the LUMA planes before it is used (MFChain.temporal_filter_run_subpel_bgr; at a boundary
    MF.cells_subpel_device on MF.frame_plane_tensor makes the copy of a grid before the planes are overwritten, so the copies hold
    the colour frames and quarter-pel grids, and MF.cells_temporal_filter_subpel_bgr_device filters)."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    if subpel_bgr and frames and frames[0].ndim != 3:
        raise ValueError("denoise_frames: subpel_bgr=True needs a colour video, (H, W, 3) frames in B,G,R order")
    if subpel and frames and frames[0].ndim == 3:
        raise _capi.BbmeError(_capi.ERR_UNSUPPORTED, "denoise_frames: subpel=True on a colour video: the BGR temporal filter rule, "
                              "the colour rule, is integer; the quarter-pel colour filter is subpel_bgr=True")
    n_pairs = len(frames) - 1
    if n_pairs < 1:
        return frames
    if device is None:
        device = local_device()
    import torch
    strength = int(strength)
    bgr = frames[0].ndim == 3
    out = [None] * len(frames)
    before, after = {}, {}                                 # frame -> copies of (previous plane, grid into it) / (frame, next plane, grid)

    def boundary(mf, g, prev, to_prev, cur, nxt, to_next):
        flt = torch.empty_like(cur)
        cells_filter = mf.cells_temporal_filter_subpel_device if subpel else mf.cells_temporal_filter_device
        bgr_filter = mf.cells_temporal_filter_subpel_bgr_device if subpel_bgr else mf.cells_temporal_filter_bgr_device
        (bgr_filter if bgr else cells_filter)(cur, prev, nxt, to_prev, to_next, strength, out=flt)
        mf.synchronize()
        keep(mf, g, flt.cpu().numpy())

    def keep(mf, g, plane):
        if bgr:                                            # the colour calls write the unpadded frame
            out[g] = np.ascontiguousarray(plane)
            return
        h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
        out[g] = np.ascontiguousarray(plane[py:py + h, px:px + w])

    def grid(mf, cur, other, cells):
        """The grid on frame `cur` = (pair, which) into frame `other` as the filter reads it: with subpel or subpel_bgr a fresh
        quarter-pel grid, refined on the GPU on the level-0 planes (in colour: the luma planes)"""
        if not (subpel or subpel_bgr):
            return cells
        q4 = mf.cells_subpel_device(mf.frame_plane_tensor(*cur), mf.frame_plane_tensor(*other), cells, out=torch.empty_like(cells))[0]
        mf.synchronize()                                   # refined on the context's stream: the copy and another context read it from theirs
        return q4

    def collect(mf, first, count):
        frame_tensor = mf.frame_bgr_tensor if bgr else mf.frame_plane_tensor
        lo = 0 if first == 0 else 1                        # the video's first frame has no previous one anywhere: the chain's own slot 0
        if count > lo:
            run = mf.temporal_filter_run_bgr if bgr else mf.temporal_filter_run_subpel if subpel else mf.temporal_filter_run
            if subpel_bgr:
                run = mf.temporal_filter_run_subpel_bgr
            for q, plane in enumerate(run(strength, lo, count - lo)):      # waits for this context's stream only
                keep(mf, first + lo + q, plane)
        else:
            mf.synchronize()
        with torch.cuda.device(device):
            # the round's first frame: its next half is here
            if first > 0:
                half = (frame_tensor(0, 0), frame_tensor(0, 1), grid(mf, (0, 0), (0, 1), mf.cells_tensor(0)))
                if first in before:
                    boundary(mf, first, *before.pop(first), *half)
                else:
                    after[first] = tuple(t.clone() for t in half)
            # the round's last frame: its previous half is here
            last = first + count
            half = (frame_tensor(count - 1, 0),
                    grid(mf, (count - 1, 1), (count - 1, 0), mf.backward_cells_tensor(count - 1)))
            if last == n_pairs:
                boundary(mf, last, *half, frame_tensor(count - 1, 1), None, None)
            elif last in after:
                boundary(mf, last, *half, *after.pop(last))
            else:
                before[last] = tuple(t.clone() for t in half)
            torch.cuda.current_stream().synchronize()      # the copies are taken before the roll and the next estimate overwrite them

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect, bidirectional=True)
    return out


def denoise_frames_wide(frames, search_size, block_size, strength, device=None, window=8, bgr=False):
    """Motion-compensated temporal denoising of a grey video on ONE GPU over TWO frames on each side (the wide temporal filter rule
    of include/bbme.h): every frame averaged with up to four motion-aligned neighbours, along quarter-pel vectors, wherever their
    2x2 cells match better than `strength` -> len(frames) unpadded uint8 (H, W) frames.  The video is cut into runs of `window`
    output frames a .. a + window - 1.  Each run gets a bidirectional chain estimate of its own over its frames plus two on
    either side, where the video has them (MFChain over frames a - 2 .. a + window + 1), and one MFChain.temporal_filter_run_wide
    over its output slots: every frame is therefore filtered from every neighbour that exists, the frames at a run's ends
    included, and a run needs nothing from another.  The price: the four pairs of a run that lie outside its own frames -- (a - 2,
    a - 1), (a - 1, a), (a + window - 1, a + window) and (a + window, a + window + 1) -- are estimated by the neighbouring run
    as well, so a video of many runs costs window + 3 pair estimates per window frames.  Runs of one length share a context.
    Without bgr a colour video is BbmeError (ERR_UNSUPPORTED): the rule is grey.  bgr=True takes a colour video only, (H, W, 3)
    frames in B,G,R order (grey frames are a ValueError), and follows the same run plan with the BGR wide temporal filter rule:
    the chains are fed the colour frames, estimate and refine on their luma planes, and one MFChain.temporal_filter_run_wide_bgr
    per run filters the stored colour -> (H, W, 3) frames.  denoise_frames is the filter over one frame on each side."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    if bgr and frames and frames[0].ndim != 3:
        raise ValueError("denoise_frames_wide: bgr=True needs a colour video, (H, W, 3) frames in B,G,R order")
    if not bgr and frames and frames[0].ndim == 3:
        raise _capi.BbmeError(_capi.ERR_UNSUPPORTED, "denoise_frames_wide: a colour video: the wide temporal filter rule is grey")
    window = int(window)
    if window < 1:
        raise ValueError("denoise_frames_wide: window must be at least 1")
    n = len(frames)
    if n < 2:
        return frames
    if device is None:
        device = local_device()
    from .motion_framework import MFChain
    out = [None] * n
    chains = {}                                            # frames of a chain -> its context
    try:
        for a in range(0, n, window):
            b = min(a + window, n)
            lo, hi = max(a - 2, 0), min(b + 2, n)
            run = frames[lo:hi]
            mf = chains.get(len(run))
            if mf is None:
                mf = chains[len(run)] = MFChain(run, search_size, block_size, device=device)
            else:
                mf.set_frame_run(0, run)
            mf.estimate_bidirectional_async()
            h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
            if bgr:                                        # the colour call writes the unpadded frame
                for q, frame in enumerate(mf.temporal_filter_run_wide_bgr(int(strength), a - lo, b - a)):
                    out[a + q] = np.ascontiguousarray(frame)
                continue
            for q, plane in enumerate(mf.temporal_filter_run_wide(int(strength), a - lo, b - a)):
                out[a + q] = np.ascontiguousarray(plane[py:py + h, px:px + w])
    finally:
        for mf in chains.values():
            mf.close()
    return out


def compose_global_models(models, unit=1):
    """Per-pair models of the global motion rule (six Q16 int32 each, grid units of 1 / unit pixel over half pixels from the plane
    centre) -> the cumulative motions (len(models) + 1, 6) float64, pixels and pixels per half pixel: row f is the displacement
    that takes a position of frame 0 to where frame 0's content lies in frame f (row 0 is zero).  Pair p's model is the map
    T_p(P) = P + 2 d_p(P) on half-pixel positions P; the cumulative map is T_{f-1} o ... o T_0, composed in double."""
    cum = np.zeros((len(models) + 1, 6), np.float64)
    A, t = np.eye(2), np.zeros(2)                          # half-pixel position in frame f = A P + t
    for f, m in enumerate(models):
        m = np.asarray(m, np.float64) / 65536.0 / unit
        Ap, tp = np.eye(2) + 2.0 * np.array([[m[1], m[2]], [m[4], m[5]]]), 2.0 * np.array([m[0], m[3]])
        A, t = Ap @ A, Ap @ t + tp
        D = (A - np.eye(2)) / 2.0
        cum[f + 1] = (t[0] / 2.0, D[0, 0], D[0, 1], t[1] / 2.0, D[1, 0], D[1, 1])
    return cum


def stabilization_corrections(models, radius=None, unit=1):
    """The correction of every frame as six Q16 int32 in pixels (unit 1 of the global compensation rule), (len(models) + 1, 6):
    radius=None locks every frame to frame 0 -- the correction is the cumulative motion --; an integer radius subtracts the
    moving average of the cumulative motions over the frames f - radius .. f + radius, the window clipped at the video's ends.
    In double, then rint(value * 65536) (half to even)."""
    cum = compose_global_models(models, unit)
    n = len(cum)
    corr = cum.copy()
    if radius is not None:
        r = int(radius)
        if r < 0:
            raise ValueError("stabilization_corrections: radius must be None or at least 0")
        for f in range(n):
            corr[f] = cum[f] - cum[max(0, f - r):min(n, f + r + 1)].mean(axis=0)
    return np.clip(np.rint(corr * 65536.0), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)


def stabilize_frames(frames, search_size, block_size, radius=None, kind="translation", tol=1.0, iterations=3, fill=0, device=None,
                     in_flight=4, batch=2):
    """Stabilisation of a grey or a colour video on ONE GPU from the dominant motion of its consecutive pairs (the global motion
    rule and the global compensation rule of include/bbme.h, for colour its BGR form) -> (frames, models, corrections):
    len(frames) unpadded uint8 frames, (H, W) or (H, W, 3) as they came, the per-pair models (P, 6) int32 (unit 1: pixels over
    half pixels from the plane centre) and the per-frame corrections (P + 1, 6) int32 each frame was warped by
    (stabilization_corrections).  The pairs are estimated on chain contexts (estimate_frames_pipelined's plan: every frame is set
    once) and every pair's model comes from MFChain.global_motion_all; the models are composed and smoothed on the host in double.
    A pixel whose source lies in the padding takes the padding's zero, one whose source lies outside the padded plane takes
    `fill`.  radius=None locks every frame to frame 0; an integer radius follows the smoothed path.
    Grey video: a copy of every frame's padded level-0 plane stays in HBM, every plane is warped by the global compensation kernel
    (MF.cells_global_compensate_device, no image 1) and the unpadded frame cut out of it.
    Colour video, (H, W, 3) frames in B,G,R order: the chains are fed the colour frames, so the models are those of the grey call
    on bgr_to_gray(video); a copy of every frame's stored colour (MF.frame_bgr_tensor) stays in HBM and no plane copy is kept;
    the frames are warped in runs of up to in_flight * batch (at most GC_MAX_FRAMES) by MF.cells_global_compensate_bgr_device,
    each run one launch under its frames' own corrections and one download."""
    import torch
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    bgr = bool(frames) and frames[0].ndim == 3
    n = len(frames)
    if n < 2:
        return frames, np.zeros((0, 6), np.int32), np.zeros((n, 6), np.int32)
    if device is None:
        device = local_device()
    models = np.zeros((n - 1, 6), np.int32)
    planes = [None] * n                                    # grey: every frame's padded plane
    store = []                                             # colour: one (n, H, W, 3) tensor of every frame's stored colour
    have = [False] * n

    def collect(mf, first, count):
        got = mf.global_motion_all(kind=kind, tol=tol, iterations=iterations)         # waits for this context's stream
        for p in range(count):
            models[first + p] = got[p]["model"]
            for which in (0, 1):
                f = first + p + which
                if have[f]:
                    continue
                have[f] = True
                if bgr:
                    src = mf.frame_bgr_tensor(p, which)
                    if not store:
                        store.append(torch.empty((n,) + tuple(src.shape), dtype=torch.uint8, device=src.device))
                    store[0][f].copy_(src)
                else:
                    planes[f] = mf.frame_plane_tensor(p, which).clone()
        torch.cuda.synchronize(device)                                                # the copies, before the planes roll

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect)
    corrections = stabilization_corrections(models, radius)
    from .motion_framework import MF, GC_MAX_FRAMES
    out = [None] * n
    mf = MF(frames[0], frames[0], search_size, block_size, len(block_size), device=device)
    try:
        h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
        if bgr:
            run = max(1, min(int(in_flight) * int(batch), GC_MAX_FRAMES, n))
            warped = torch.empty((run, h, w, 3), dtype=torch.uint8, device=store[0].device)
            for f0 in range(0, n, run):
                k = min(run, n - f0)
                mf.cells_global_compensate_bgr_device(None, store[0][f0:f0 + k], corrections[f0:f0 + k], unit=1, out=warped[:k], fill=fill)
                mf.synchronize()
                host = warped[:k].cpu().numpy()
                for i in range(k):
                    out[f0 + i] = np.ascontiguousarray(host[i])
        else:
            warped = torch.empty((mf.padded_height, mf.padded_width), dtype=torch.uint8, device=planes[0].device)
            for f in range(n):
                mf.cells_global_compensate_device(None, planes[f], corrections[f], unit=1, out=warped, fill=fill)
                mf.synchronize()
                out[f] = np.ascontiguousarray(warped.cpu().numpy()[py:py + h, px:px + w])
    finally:
        mf.close()
    return out, models, corrections


def predict_frames(frames, search_size, block_size, subpel=True, in_flight=4, batch=2, device=None):
    """The motion-compensated prediction of every frame of a video from the next one, and its residual, on ONE GPU ->
    (predictions, stats): for every consecutive pair (f_k, f_k+1) the prediction of f_k from f_k+1 along the pair's field, an
    unpadded uint8 frame shaped as the frames came, and stats (P, 4) uint64, row k = (sse, sad, pixels, skipped) of that
    prediction against f_k over the unpadded frame.  On the chain plan of estimate_frames_pipelined (every frame is set once);
    a round's statistics come from one launch over its pairs.  subpel=True predicts along the cells refined to quarter pels on
    the level-0 (luma) planes, subpel=False along the integer cells.
    Grey video: the unpadded crop of MF.draw_MVimage_subpel / draw_MVimage(0, 2) and the statistics of
    compensation_errors_subpel / compensation_errors over the unpadded frame.
    Colour video, (H, W, 3) frames in B,G,R order: the chains are fed the colour frames, so the fields are those of the grey
    call on bgr_to_gray(video); predictions and statistics are the BGR compensation rule's on the stored colour
    (get_pair_motion_compensated_bgr, compensation_errors_bgr), sse and sad summed over the three channels."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    n_pairs = len(frames) - 1
    if n_pairs < 1:
        return [], np.zeros((0, 4), np.uint64)
    bgr = frames[0].ndim == 3
    if device is None:
        device = local_device()
    out = [None] * n_pairs
    stats = np.zeros((n_pairs, 4), np.uint64)

    def collect(mf, first, count):
        h, w, py, px = mf.orig_height, mf.orig_width, mf.padding_y, mf.padding_x
        if bgr:
            errors = mf.compensation_errors_bgr(unit=4 if subpel else 1)              # waits for this context's stream only
        else:
            errors = mf.compensation_errors_subpel() if subpel else mf.compensation_errors(0, 2)
        for p in range(count):
            if bgr:
                out[first + p] = mf.get_pair_motion_compensated_bgr(p, unit=4 if subpel else 1)
            else:
                plane = mf.get_pair_motion_compensated_subpel(p) if subpel else mf.get_pair_motion_compensated(p, 0, 2)
                out[first + p] = np.ascontiguousarray(plane[py:py + h, px:px + w])
            stats[first + p] = [errors[p][k] for k in ("sse", "sad", "pixels", "skipped")]

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect)
    return out, stats


def colorize_frames(frames, search_size, block_size, maxmotion=-1.0, scale=1, in_flight=4, batch=2, device=None):
    """The colour-coded forward field of the len(frames) - 1 consecutive pairs of a video on ONE GPU (the colour rule of
    include/bbme.h at subsampling `scale`): -> ((P, oh, ow, 3) uint8 B,G,R images, (P, 5) float32 ranges (max radius, min u,
    max u, min v, max v)).  maxmotion > 0 normalises every picture by the same radius; otherwise each by its own.  Runs on the
    chain plan of estimate_frames_pipelined (same contexts, rounds and padding of a short round): every frame is set once, a
    round's ranges come from one launch (MFBatch.flow_ranges_all) and only the images' bytes are downloaded."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    n_pairs = len(frames) - 1
    if n_pairs < 1:
        return np.empty((0, 0, 0, 3), np.uint8), np.empty((0, 5), np.float32)
    if device is None:
        device = local_device()
    images = [None] * n_pairs
    ranges = np.empty((n_pairs, 5), np.float32)

    def collect(mf, first, count):
        ranges[first:first + count] = mf.flow_ranges_all("forward", scale)[:count]      # waits for this context's stream only
        for p in range(count):
            images[first + p] = mf.get_pair_flow_color(p, scale, maxmotion)

    _walk_chains(frames, search_size, block_size, device, in_flight, batch, collect)
    return np.stack(images), ranges


def _gpu_compute(search_size, block_size, device):
    from .motion_framework import MF

    def run(frame1, frame2):
        mf = MF(frame1, frame2, search_size, block_size, len(block_size), device=device)
        try:
            flow = mf.calcMotionBlockMatching()
            py, px = mf.padding_y, mf.padding_x
            h, w = frame1.shape
            return np.ascontiguousarray(flow[py:py + h, px:px + w])
        finally:
            mf.close()
    return run


def estimate_sequence(pairs, search_size, block_size, n_pairs=None, out_dir=None, compute=None,
                      device=None, group=None):
    """Run the local shard and gather every pair's (H, W, 2) float32 field on rank 0.

    pairs    : dict {global_pair_index: (frame1, frame2)} holding at least this rank's shard
    compute  : callable (frame1, frame2) -> unpadded (H, W, 2) float32 flow; default = the HIP path
    Returns the list of all fields in pair order on rank 0 (and writes NNNN.flo files into out_dir
    when given), None on the other ranks.
    """
    import torch
    import torch.distributed as dist
    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank(group) if distributed else 0
    world = dist.get_world_size(group) if distributed else 1
    if n_pairs is None:
        n_pairs = max(pairs) + 1
    if device is None:
        device = local_device()                           # one process per GPU: never every rank on cuda:0
    if compute is None:
        compute = _gpu_compute(search_size, block_size, device)
    mine = shard_pairs(n_pairs, rank, world)
    local = {p: compute(*pairs[p]) for p in mine}
    results = None
    if not distributed or world == 1:
        results = [local[p] for p in range(n_pairs)]
    else:
        on_gpu = dist.get_backend(group) == "nccl"
        dev = torch.device("cuda", device) if on_gpu else torch.device("cpu")
        rounds = (n_pairs + world - 1) // world
        results = [None] * n_pairs if rank == 0 else None
        shape = next(iter(local.values())).shape if local else None
        shapes = [None] * world
        dist.all_gather_object(shapes, shape, group=group)
        shape = next(s for s in shapes if s is not None)
        for k in range(rounds):                           # one gather per round of `world` pairs
            p = k * world + rank
            t = torch.from_numpy(local[p]).to(dev) if p < n_pairs else torch.zeros(shape, dtype=torch.float32, device=dev)
            bucket = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(world)] if rank == 0 else None
            dist.gather(t, bucket, dst=0, group=group)
            if rank == 0:
                for r in range(world):
                    q = k * world + r
                    if q < n_pairs:
                        results[q] = bucket[r].cpu().numpy()
    if rank == 0 and out_dir is not None:
        from .rw_flow import Flow
        os.makedirs(out_dir, exist_ok=True)
        for p, f in enumerate(results):
            Flow().WriteFlowFile(f, os.path.join(out_dir, "%04d.flo" % p))
    return results if rank == 0 else None
