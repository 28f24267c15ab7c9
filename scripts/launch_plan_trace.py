#!/usr/bin/env python3
"""The launches of an estimate, as a kernel trace shows them, against the launch plan (csrc/launch_plan.hpp).

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python scripts/launch_plan_trace.py --run      (on the GPU)
    python scripts/launch_plan_trace.py --compare OUT [OTHER_OUT ...]                                      (offline)

--run makes one estimate per context of CONTEXTS, in order.  --compare prints, per context, the plan (the dump of
tests/cpp/launch_plan_test.cpp under the context's knobs) and checks every trace against it: the kernels of the main stream in the
plan's order with the plan's grid and workgroup, and the speculative searches of the side stream among them (a trace is sorted by
start time, and a speculative search starts somewhere beside the sweeps behind its fork).  The trace's LDS_Block_Size is the
kernel's STATIC LDS (k_search_fast shows 0 with 17 408 bytes of dynamic LDS), so the plan's dynamic LDS is not in a trace and is
not compared.  Given several traces it also compares them with each other launch by launch: name, grid, workgroup and the LDS
column as the trace has it."""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_ALL = {"BBME_SPEC_MIN_GABS": "0"}
# name, kind, width, height, search, block, dump options, environment of the context
CONTEXTS = [
    ("cfg3", "single", 3840, 2160, [80] * 4, [16] * 4, {}, {}),
    ("cfg4", "single", 3840, 2160, [72] * 4, [8] * 4, {}, {}),
    ("cfg2", "single", 1920, 1080, [48] * 3, [16] * 3, {}, {}),
    ("cfg1", "single", 584, 388, [30] * 3, [16] * 3, {}, {}),
    ("ref", "single", 2336, 1552, [64] * 4, [32] * 4, {}, {}),
    ("cfg3_batch6", "batch", 3840, 2160, [80] * 4, [16] * 4, {"pairs": 6}, {}),
    ("small_b16_spec", "single", 512, 384, [48, 48, 48], [16, 16, 16], {}, SPEC_ALL),
    ("small_b8_spec", "single", 384, 256, [72, 72], [8, 8], {}, SPEC_ALL),
    ("batch3_spec", "batch", 512, 384, [48, 48, 48], [16, 16, 16], {"pairs": 3}, SPEC_ALL),
    ("chain3", "chain", 584, 388, [30] * 3, [16] * 3, {"pairs": 3, "chain": 1}, {}),
    ("backward", "backward", 584, 388, [32, 32, 42], [16, 16, 32], {}, SPEC_ALL),
    ("jacobi", "jacobi", 512, 384, [48, 48, 48], [16, 16, 16], {"jacobi": 1}, SPEC_ALL),
    ("raster", "raster", 352, 256, [48, 40, 40], [16, 16, 8], {"raster": 1}, SPEC_ALL),
    ("no_graph", "single", 1920, 1080, [48] * 3, [16] * 3, {}, {"BBME_NO_GRAPH": "1"}),
]


def run():
    sys.path.insert(0, ROOT)
    import blockbasedmotionestimation_amd as bbme
    for name, kind, w, h, search, block, opts, env in CONTEXTS:
        os.environ.update(env)
        try:
            pairs = [bbme.synth_pair(w, h, 1900 + p, max_motion=12)[:2] for p in range(opts.get("pairs", 1))]
            if kind == "batch":
                mf = bbme.MFBatch(pairs, search, block, len(block))
            elif kind == "chain":
                mf = bbme.MFChain([pairs[p % 2][p // 2 % 2] for p in range(len(pairs) + 1)], search, block, len(block))
            else:
                mf = bbme.MF(pairs[0][0], pairs[0][1], search, block, len(block))
        finally:
            for key in env:
                del os.environ[key]
        if kind == "backward":
            mf.set_direction(True)
        if kind == "jacobi":
            mf.set_regularizer_mode(True)
        if kind == "raster":
            mf.set_search_mode(True)
        mf.estimate_async()
        mf.synchronize()
        mf.close()
        print("estimated", name, flush=True)


def dump_exe(workdir):
    exe = os.path.join(workdir, "launch_plan_test")
    csrc = os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cpp", "launch_plan_test.cpp"), os.path.join(csrc, "bbme_host.cpp"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    return exe


STATIC_LDS = set()                                 # (kernel, the trace's LDS column) seen on the main stream
LAUNCH = re.compile(r"^(\S.*\S) grid=(\d+)x(\d+) wg=(\d+) lds=(\d+) stream=(main|side)$")


def planned(exe, ctx):
    """[(kernel, threads x, grid y, workgroup, dynamic LDS, stream)] of the context's estimate"""
    name, kind, w, h, search, block, opts, env = ctx
    cmd = [exe, "dump", str(w), str(h), ",".join(map(str, search)), ",".join(map(str, block))] + ["%s=%d" % kv for kv in opts.items()]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BBME_")}
    out = subprocess.run(cmd, env=dict(clean, **env), check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    launches = []
    for line in out.splitlines():
        m = LAUNCH.match(line)
        if m:
            k, gx, gy, wg, lds, stream = m.groups()
            launches.append((k.replace(" ", ""), int(gx) * int(wg), int(gy), int(wg), int(lds), stream))
    return out, launches


def traced(outdir):
    """The trace's estimates: per k_expand, the launches of the plan's kernels up to it, by start time"""
    f = max(glob.glob(outdir + "/**/*kernel_trace.csv", recursive=True), key=os.path.getmtime)
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    estimates, cur = [], []
    for r in rows:
        k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("bbme::", "").replace(" ", "")
        if not k.startswith(("k_search", "k_fixup", "k_reg", "k_expand")):
            continue
        cur.append((k, int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Workgroup_Size_X"]), int(r["LDS_Block_Size"])))
        if k == "k_expand":
            estimates.append(cur)
            cur = []
    return estimates


def against_plan(plan, trace):
    """'' or what differs.  The side stream's launches may lie anywhere in the trace."""
    side = [p for p in plan if p[5] == "side"]
    rest = list(trace)
    for p in side:
        hit = [i for i, t in enumerate(rest) if t[:4] == p[:4]]
        if not hit:
            return "the speculative launch %s is not in the trace" % (p,)
        del rest[hit[0]]
    main = [p for p in plan if p[5] == "main"]
    if len(main) != len(rest):
        return "%d launches planned on the main stream, %d traced" % (len(main), len(rest))
    for i, (p, t) in enumerate(zip(main, rest)):
        if p[:4] != t[:4]:
            return "launch %d: planned %s, traced %s" % (i, p, t)
        STATIC_LDS.add((p[0].split("<")[0], t[4]))
    return ""


def compare(outdirs):
    with tempfile.TemporaryDirectory() as tmp:
        exe = dump_exe(tmp)
        plans = [planned(exe, ctx) for ctx in CONTEXTS]
    traces = [traced(d) for d in outdirs]
    bad = 0
    for d, tr in zip(outdirs, traces):
        if len(tr) != len(CONTEXTS):
            print("%s: %d estimates traced, %d contexts" % (d, len(tr), len(CONTEXTS)))
            return 1
    for i, ctx in enumerate(CONTEXTS):
        text, plan = plans[i]
        print("== %s: %d launches planned ==" % (ctx[0], len(plan)))
        for d, tr in zip(outdirs, traces):
            diff = against_plan(plan, tr[i])
            bad += bool(diff)
            print("  %s: %d launches traced, %s" % (d, len(tr[i]), diff or "as planned"))
        for d, tr in zip(outdirs[1:], traces[1:]):
            same = sorted(tr[i]) == sorted(traces[0][i]) and [t for t in tr[i] if "k_search_fast" not in t[0] and "k_search_generic" not in t[0]] == \
                   [t for t in traces[0][i] if "k_search_fast" not in t[0] and "k_search_generic" not in t[0]]
            bad += not same
            print("  %s against %s: %s" % (d, outdirs[0], "the same launches (name, grid, workgroup, LDS column), the same order" if same else "DIFFERENT"))
    print("the trace's LDS column (static LDS), per kernel: " + ", ".join("%s %d" % kv for kv in sorted(STATIC_LDS)))
    print("RESULT: %s" % ("%d differences" % bad if bad else "every trace as planned, all traces alike"))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--run"]:
        run()
    elif sys.argv[1:2] == ["--compare"] and len(sys.argv) > 2:
        sys.exit(compare(sys.argv[2:]))
    else:
        sys.exit(__doc__)
