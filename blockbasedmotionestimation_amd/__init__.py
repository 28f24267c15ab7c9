"""MI355X-native block-matching motion estimation (hot path of ashish-nr/BlockBasedMotionEstimation).

The compute path is hand-written HIP for gfx950 behind the C-ABI of include/bbme.h
(libbbme.so, built in-tree by `python -m blockbasedmotionestimation_amd.build`).
MF and Flow mirror the reference's classes; there is no CPU fallback.
"""
from ._capi import BbmeError, LIB_PATH  # noqa: F401
from .motion_framework import (MF, MFBatch, MFChain, plan_padding, pad_zero, pyr_down, resize_x4, cells_consistency,  # noqa: F401
                               interpolate_cells, color_cells, bgr_to_gray, interpolate_cells_bgr, temporal_filter_cells,
                               temporal_filter_cells_bgr, subpel_cells, compensate_cells_subpel, interpolate_cells_subpel,
                               interpolate_cells_subpel_bgr, temporal_filter_cells_subpel, temporal_filter_cells_subpel_bgr,
                               compose_cells, temporal_filter_cells_wide, temporal_filter_cells_wide_bgr, vector_histogram_cells,
                               global_moments_cells,
                               solve_global_motion, global_motion_cells, global_compensate, global_compensate_bgr,
                               compensate_cells_bgr,
                               DIR_FORWARD, DIR_BACKWARD, FB_CONSISTENT, FB_INCONSISTENT, FB_OUTSIDE)
from .rw_flow import Flow, FlowWriter, subsample_div4  # noqa: F401
from .synth import synth_pair, synth_video, warp_pair_from_flow  # noqa: F401

__all__ = ["MF", "MFBatch", "MFChain", "Flow", "FlowWriter", "BbmeError", "plan_padding", "pad_zero", "pyr_down", "resize_x4",
           "subsample_div4", "synth_pair", "synth_video", "warp_pair_from_flow", "cells_consistency", "DIR_FORWARD", "DIR_BACKWARD",
           "FB_CONSISTENT", "FB_INCONSISTENT", "FB_OUTSIDE", "interpolate_cells", "color_cells", "bgr_to_gray", "interpolate_cells_bgr",
           "temporal_filter_cells", "temporal_filter_cells_bgr", "subpel_cells", "compensate_cells_subpel",
           "interpolate_cells_subpel", "interpolate_cells_subpel_bgr", "temporal_filter_cells_subpel",
           "temporal_filter_cells_subpel_bgr", "compose_cells", "temporal_filter_cells_wide", "temporal_filter_cells_wide_bgr",
           "vector_histogram_cells",
           "global_moments_cells", "solve_global_motion", "global_motion_cells", "global_compensate", "global_compensate_bgr",
           "compensate_cells_bgr"]
