#!/usr/bin/env python3
"""Generates the committed fixtures under tests/golden/.  Run in the build container:

    python tests/golden/make_golden.py

1. hotpath_*.npz -- inputs (level planes AFTER padding + pyramid) and expected outputs of the hot
   path (MV grid after the search of every level and after every regulariser sweep, final dense
   flow) for small seeded cases.  Written by the CPU oracle (oracle/bbme_oracle.c) and PINNED: step 6
   has the reference's own compiled core compute every stage of them again (variant_jacobi_* is not a
   reference function and stays the oracle's).
2. flo_ramp_ref.flo -- a 7x5 .flo written by the REFERENCE's own Middlebury code
   (middlebury/flow-code/flowIO.cpp, compiled into oracle/_ref/flo_ref): pins the codec.
3. gt_stats.json -- known answers computed with the reference's own reader on the 8 ground-truth
   files it ships (size, unknown-pixel count, sums, sha256), plus the Venus file (the smallest) as
   data, gzipped (gt_Venus_flow10.flo.gz; the .flo itself is larger than a committed file may be),
   so that the known-answer tests need no copy of the reference.
4. color_ref.npz -- colour coding made by the REFERENCE's own vendored colour-wheel code
   (middlebury/flow-code/colorcode.cpp computeColor, compiled into oracle/_ref/flo_ref, called by
   oracle/ref_flo_driver.cpp): Venus ground truth with the automatic radius and with maxmotion 3.5
   (exercises the out-of-range branch), and a synthetic wheel field (all angles, radii 0..1.5,
   some unknown pixels).  gt_stats.json also gets the sha256 of that output for all 8 GT files.
5. gt_samples.npz -- every GT_STRIDE-th row and column of each of the 8 GT files (the whole files are
   too large to commit), written by the oracle and read + rewritten by the REFERENCE's flowIO.cpp
   (flo_ref roundtrip; the bytes must come back unchanged), with the reference's stats of the sample
   and its colour coding (flo_ref color, automatic radius).  `python tests/golden/make_golden.py
   gt_samples` rewrites this file alone.
6. reference_digests.json -- sha256 of what the REFERENCE's own core (motion_framework.cpp compiled in place
   into oracle/_ref/mf_ref, see oracle/Makefile) computes: every stage and the dense field of the hotpath_* /
   variant_raster_* files above (the step fails if a file differs from the reference), and the inputs, stages,
   sweeps, fields and motion-compensated frames of the cases of tests/test_gpu_reference.py (tests/helpers.py:
   REF_*).  `python tests/golden/make_golden.py reference_digests` rewrites this file alone.
"""
import gzip
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import bbme_oracle as O                                     # noqa: E402
from blockbasedmotionestimation_amd.synth import synth_pair             # noqa: E402
import helpers as H                                                     # noqa: E402
from helpers import oracle_schedule                                     # noqa: E402

REF = "/root/reference"

CASES = {
    # name: (w, h, search, block, seed, max_motion)
    "hotpath_b16_r7_l3": (160, 112, [30, 30, 30], [16, 16, 16], 2001, 6),
    "hotpath_b16_r16_l2": (128, 96, [48, 48], [16, 16], 2002, 12),
    "hotpath_b8_r32_l2": (96, 64, [72, 72], [8, 8], 2003, 10),
    "hotpath_b32_r16_l2": (256, 128, [64, 64], [32, 32], 2004, 14),
    "hotpath_mixed_l3": (192, 128, [24, 40, 30], [8, 16, 8], 2005, 8),
    # the reference's second literal set (main_class.cpp:15-17): block {16,16,32}, search {32,32,42}; 376 x 250 pads to 384 x 256
    "hotpath_ref2_l3": (376, 250, [32, 32, 42], [16, 16, 32], 2006, 8),
    # 2 x 2 blocks as a level's own block size (level 0 here), under 4 x 4
    "hotpath_block2_l2": (96, 64, [12, 16], [2, 4], 2007, 5),
}


# the variants of SURVEY 8(f4): "variant_*.npz", made with `python tests/golden/make_golden.py variants` (the files above
# are not rewritten).  raster: MF::find_min_block (:246-294) as the search; jacobi: NOT the reference -- the product's
# opt-in fast regulariser as the oracle defines it.
VARIANTS = {
    "variant_raster_b16_r7_l3": (160, 112, [30, 30, 30], [16, 16, 16], 2101, 6, "raster"),
    "variant_raster_b8_r32_l2": (96, 64, [72, 72], [8, 8], 2102, 10, "raster"),
    "variant_jacobi_b16_r7_l3": (160, 112, [30, 30, 30], [16, 16, 16], 2103, 6, "jacobi"),
}


def make_hotpath(name, w, h, search, block, seed, mm, mode=None):
    f1, f2, _ = synth_pair(w, h, seed, max_motion=mm)
    L = len(block)
    omf = O.OracleMF(f1, f2, search, block)
    if mode == "raster":
        omf.set_raster_search(True)
    if mode == "jacobi":
        omf.set_jacobi_regularizer(True)
    data = {"search_size": np.array(search, np.int32), "block_size": np.array(block, np.int32),
            "frame1": f1, "frame2": f2,
            "geometry": np.array([omf.padded_width, omf.padded_height, omf.padding_x, omf.padding_y], np.int32)}
    for lvl in range(L):
        data["plane1_l%d" % lvl] = omf.image(lvl, 1).copy()
        data["plane2_l%d" % lvl] = omf.image(lvl, 2).copy()
    stages = []

    def on_stage(kind, lvl, b, mvs):
        key = "mv_%02d_%s_l%d_b%d" % (len(stages), kind, lvl, b)
        stages.append(key)
        data[key] = mvs.astype(np.int16)

    data["flow"] = oracle_schedule(omf, L, on_stage)
    data["stages"] = np.array(stages)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **data)
    print(name, "stages:", len(stages), "flow", data["flow"].shape)


def wheel_field():
    """All angles and radii 0 .. 1.5 of the normalising radius, a band of unknown pixels, signed zeros."""
    y, x = np.mgrid[-60:61, -90:91].astype(np.float32)
    f = np.stack([x * np.float32(0.37), y * np.float32(0.53)], -1).astype(np.float32)
    f[5:9, :, 0] = 1e10                                    # unknown (rw_flow.cpp:39-43)
    f[60, :, 1] = -0.0                                     # atan2 of a negative zero: the +pi / -pi seam
    return f


GT_STRIDE = 8


def make_gt_samples(flo_ref, gt_dir):
    data = {}
    tmp = tempfile.mkdtemp(prefix="bbme_gt_")
    mine, ref = os.path.join(tmp, "sample.flo"), os.path.join(tmp, "sample_ref.flo")
    for seq in sorted(os.listdir(gt_dir)):
        sample = O.flo_read(os.path.join(gt_dir, seq, "flow10.flo"))[::GT_STRIDE, ::GT_STRIDE]
        O.flo_write(mine, sample)
        subprocess.check_call([flo_ref, "roundtrip", mine, ref])
        raw = open(ref, "rb").read()
        assert raw == open(mine, "rb").read(), seq
        w, h, unk, su, sv = subprocess.check_output([flo_ref, "stats", ref]).decode().split()
        assert (int(h), int(w)) == sample.shape[:2]
        data[seq + "_flo"] = np.frombuffer(raw, np.uint8)
        data[seq + "_unknown"] = np.array(int(unk), np.int64)
        data[seq + "_sums"] = np.array([float(su), float(sv)], np.float64)
        data[seq + "_color"] = color_by_reference(flo_ref, ref, sample.shape[:2])
    shutil.rmtree(tmp)
    np.savez_compressed(os.path.join(HERE, "gt_samples.npz"), stride=np.array(GT_STRIDE, np.int64), **data)
    print("gt samples:", {k[:-4]: v.shape for k, v in data.items() if k.endswith("_flo")})


def color_by_reference(flo_ref, flo_path, shape, maxmotion=None):
    out = os.path.join("/tmp", "bbme_color_ref.bgr")
    cmd = [flo_ref, "color", flo_path, out] + ([repr(maxmotion)] if maxmotion else [])
    subprocess.check_call(cmd)
    return np.fromfile(out, np.uint8).reshape(shape[0], shape[1], 3)


def grid_digest(grid):
    """sha256 of a float32 grid of the reference as int16 (what bbme_stage_get_mvs hands out)."""
    assert np.array_equal(grid, np.round(grid)) and grid.min() >= -32768 and grid.max() <= 32767, "not an int16 grid"
    return H.sha256_of(grid.astype(np.int16))


def stage_record(planes1, planes2, search, block, raster=False):
    ref = O.ref_stages(planes1[0], planes2[0], search, block, planes=(planes1, planes2), mode="raster" if raster else None)
    whole = ref["flow"] if raster else ref["whole"]
    assert whole.tobytes() == ref["flow"].tobytes()
    rec = {"inputs": H.sha256_of(np.array(search + block, np.int32), *(list(planes1) + list(planes2))),
           "stages": [[H.stage_key(n, l, b), grid_digest(g)] for n, l, b, g in ref["stages"]],
           "flow": H.sha256_of(whole.astype(np.float32))}
    return rec, ref


def make_reference_digests():
    assert O.have_mf_ref(), "oracle/_ref/mf_ref missing (needs the reference)"
    out = {"golden": {}, "stages": {}, "spec": {}, "random": {}, "sweeps": {}, "coarse": {}, "mc": {}}
    for name in sorted(list(CASES) + [v for v in VARIANTS if "raster" in v]):
        g = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
        L = len(g["block_size"])
        p1, p2 = [g["plane1_l%d" % l] for l in range(L)], [g["plane2_l%d" % l] for l in range(L)]
        ref = O.ref_stages(g["frame1"], g["frame2"], g["search_size"].tolist(), g["block_size"].tolist(), planes=(p1, p2),
                           mode="raster" if "raster" in name else None)
        keys = [str(k) for k in g["stages"]]
        assert len(keys) == len(ref["stages"]) and list(ref["geometry"]) == g["geometry"].tolist(), name
        for key, (_, _, _, grid) in zip(keys, ref["stages"]):
            assert np.array_equal(grid, g[key].astype(np.float32)), "%s %s: the reference disagrees with the file" % (name, key)
        whole = ref["flow"] if ref["whole"] is None else ref["whole"]
        assert whole.tobytes() == g["flow"].tobytes() == ref["flow"].tobytes(), name
        out["golden"][name] = {"inputs": H.sha256_of(np.concatenate([p.reshape(-1) for p in p1 + p2])),
                               "stages": [[k, grid_digest(r[3])] for k, r in zip(keys, ref["stages"])],
                               "flow": H.sha256_of(whole.astype(np.float32))}
    for name in H.REF_STAGE_CASES:
        p1, p2, search, block, raster = H.ref_stage_case(O, name)
        out["stages"][name], ref = stage_record(p1, p2, search, block, raster)
        if name == H.REF_MC_CASE:
            finals = {l: g for n, l, b, g in ref["stages"] if (n, b) == ("sweep2", 2)}
            for lvl in range(len(block)):
                for b in sorted({2, 8, block[lvl]}):
                    grid = finals[lvl][::b // 2, ::b // 2]
                    frames = [O.ref_mc(p2[lvl], b, grid, fill) for fill in H.REF_MC_FILLS]
                    out["mc"]["l%d_b%d" % (lvl, b)] = {"frames": [H.sha256_of(f) for f in frames],
                                                       "stats": H.mc_stats(p1[lvl], frames[0], frames[1])}
    for name in H.REF_SPEC_CASES:
        c = H.LIMIT_CONTENTS[name]
        p1, p2 = H.limit_content_planes(name)
        out["spec"][name], _ = stage_record(p1, p2, c["search"], c["block"])
    for seed in H.REF_RANDOM_SEEDS:
        p1, p2, search, block = H.ref_random_case(O, seed)
        out["random"][str(seed)], _ = stage_record(p1, p2, search, block)
    g = H.ENERGY_LEVEL
    for b in H.ENERGY_BLOCKS:
        for kind in H.ENERGY_FIELDS:
            p1, p2, field = H.energy_case(b, kind)
            for run, mults in enumerate(H.ENERGY_RUNS):
                sweeps = O.ref_sweeps(p1[0], p2[0], g["search"][0], g["block"][0], b, field, mults)
                out["sweeps"]["energy_b%d_%s_run%d" % (b, kind, run)] = {"inputs": H.sha256_of(p1[0], p2[0], field),
                                                                        "sweeps": [grid_digest(s) for s in sweeps]}
    g = H.INT16_LEVELS
    for b in (16, 8, 2):
        p1, p2, field = H.int16_case(b)
        sweeps = O.ref_sweeps(p1[1], p2[1], g["search"][1], g["block"][1], b, field)
        out["sweeps"]["int16_b%d" % b] = {"inputs": H.sha256_of(p1[0], p2[0], p1[1], p2[1], field),
                                          "sweeps": [grid_digest(s) for s in sweeps]}
        if b == 2:
            for k, grid in enumerate((field, sweeps[1].astype(np.int16))):
                out["coarse"]["int16_from_%s" % ("field", "sweeps")[k]] = grid_digest(
                    O.ref_search_from_coarse(p1, p2, g["search"], g["block"], grid))
    with open(os.path.join(HERE, "reference_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("reference digests:", {k: len(v) for k, v in out.items()})


def main():
    O.build(force=True)
    if sys.argv[1:] == ["reference_digests"]:
        make_reference_digests()
        return
    if sys.argv[1:] == ["variants"]:
        for name, cfg in VARIANTS.items():
            make_hotpath(name, *cfg)
        return
    if sys.argv[1:] == ["gt_samples"]:
        assert os.path.exists(O.FLO_REF), "oracle/_ref/flo_ref missing (needs the reference)"
        make_gt_samples(O.FLO_REF, os.path.join(REF, "middlebury", "gt-flow"))
        return
    if len(sys.argv) == 3 and sys.argv[1] == "only":          # one hot-path case; the other files are not rewritten
        make_hotpath(sys.argv[2], *{**CASES, **VARIANTS}[sys.argv[2]])
        return
    for name, cfg in CASES.items():
        make_hotpath(name, *cfg)
    flo_ref = O.FLO_REF
    assert os.path.exists(flo_ref), "oracle/_ref/flo_ref missing (needs /root/reference)"
    subprocess.check_call([flo_ref, "ramp", "7", "5", os.path.join(HERE, "flo_ramp_ref.flo")])
    stats = {}
    gt_dir = os.path.join(REF, "middlebury", "gt-flow")
    for seq in sorted(os.listdir(gt_dir)):
        p = os.path.join(gt_dir, seq, "flow10.flo")
        w, h, unk, su, sv = subprocess.check_output([flo_ref, "stats", p]).decode().split()
        stats[seq] = {"width": int(w), "height": int(h), "unknown": int(unk), "sum_u": float(su), "sum_v": float(sv),
                      "bytes": os.path.getsize(p), "sha256": hashlib.sha256(open(p, "rb").read()).hexdigest()}
        shape = (int(h), int(w))
        stats[seq]["color_sha256"] = hashlib.sha256(color_by_reference(flo_ref, p, shape).tobytes()).hexdigest()
    json.dump(stats, open(os.path.join(HERE, "gt_stats.json"), "w"), indent=1, sort_keys=True)
    venus = os.path.join(gt_dir, "Venus", "flow10.flo")
    vshape = (stats["Venus"]["height"], stats["Venus"]["width"])
    wheel = wheel_field()
    wheel_path = "/tmp/bbme_wheel.flo"
    O.flo_write(wheel_path, wheel)
    np.savez_compressed(os.path.join(HERE, "color_ref.npz"),
                        venus_auto=color_by_reference(flo_ref, venus, vshape),
                        venus_max3p5=color_by_reference(flo_ref, venus, vshape, 3.5),
                        wheel_flow=wheel,
                        wheel_auto=color_by_reference(flo_ref, wheel_path, wheel.shape),
                        wheel_max40=color_by_reference(flo_ref, wheel_path, wheel.shape, 40.0))
    with open(venus, "rb") as src, open(os.path.join(HERE, "gt_Venus_flow10.flo.gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=9, mtime=0) as dst:
            shutil.copyfileobj(src, dst)
    make_gt_samples(flo_ref, gt_dir)
    make_reference_digests()
    print("gt stats:", {k: (v["width"], v["height"], v["unknown"]) for k, v in stats.items()})


if __name__ == "__main__":
    main()
