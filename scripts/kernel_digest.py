#!/usr/bin/env python3
"""Fingerprint of the device code of libbbme.so, to show that a host-side change left the kernels alone.

    python scripts/kernel_digest.py [--source bbme_device.hip | --code-object file.co] [--out digest.txt]

Compiles the device side of csrc/bbme_device.hip alone (the library's flags plus --cuda-device-only -c), takes the gfx950
code object out of the bundle and prints, per function symbol: name, size in bytes, for kernels the resources of the
code object's metadata (VGPRs, SGPRs, LDS, scratch, SGPR / VGPR spills) and a hash of its instructions.  Two builds have
the same kernels when `diff` of their outputs is empty.

The hash is over the disassembly without addresses, with ONE operand masked: the 32-bit literal of the s_add_u32 that
follows an s_getpc_b64.  It is the distance from that instruction to its target (.rodata, or another function), so it
changes when functions are merely placed in another order -- which the order of first template instantiation on the
host side decides.  Everything else in a function is position-independent.  The `s_nop 0` lines (and the `...` of a zero fill) that the disassembler
prints between a function's last instruction and the next symbol are alignment padding, as many as the placement of the
NEXT function needs: they are outside the symbol's size and are not hashed.  No GPU needed.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc")
ARCH = "gfx950"
KERNEL_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
               ".sgpr_spill_count", ".vgpr_spill_count")


def _tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name)):
        if os.path.exists(cand):
            return cand
    raise RuntimeError(name + " not found under " + rocm)


def _run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def code_object(source, workdir):
    sys.path.insert(0, ROOT)
    from blockbasedmotionestimation_amd import build as _build
    obj, co = os.path.join(workdir, "dev.o"), os.path.join(workdir, "dev.co")
    subprocess.check_call([_build._hipcc(), "--offload-arch=" + ARCH, "-std=c++17", "-O3", "-fPIC", "-Wall", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "hip", "--cuda-device-only", "-c", source, "-o", obj])
    subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o",
                           "--targets=hip-amdgcn-amd-amdhsa--" + ARCH, "--input=" + obj, "--output=" + co])
    return co


def functions(co):
    """name -> size of every FUNC symbol, and the set of kernels (the symbols with a kernel descriptor NAME.kd)"""
    funcs, kds = {}, set()
    for line in _run(_tool("llvm-readelf"), "--symbols", "--wide", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            funcs[f[7]] = int(f[2])
        elif len(f) == 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
            kds.add(f[7][:-3])
    return funcs, kds


def resources(co):
    """kernel symbol -> the KERNEL_KEYS of the code object's metadata note"""
    out, cur = {}, {}
    for line in _run(_tool("llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", line)       # kernel level only: arguments sit deeper
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip("'\"")
        if m.group(2) == ".symbol":
            out[cur[".symbol"][:-3]] = cur
    return out


def code_hashes(co):
    """function symbol -> sha256 of its instructions, placement masked (see the module's docstring)"""
    hashes, name, h, after_getpc, held = {}, None, None, False, b""
    for line in _run(_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            if name:
                hashes[name] = h.hexdigest()
            name, h, after_getpc, held = m.group(1), hashlib.sha256(), False, b""
            continue
        if name is None or not line.startswith("\t"):
            continue
        insn = " ".join(line.split("//")[0].split())
        if after_getpc:
            insn = re.sub(r"^(s_add_u32 s\d+, s\d+,) \S+$", r"\1 <pc-relative>", insn)
        after_getpc = insn.startswith("s_getpc_b64")
        if insn in ("s_nop 0", "..."):                            # hashed only once an instruction follows: a trailing run is padding
            held += insn.encode() + b"\n"
            continue
        h.update(held + insn.encode() + b"\n")
        held = b""
    if name:
        hashes[name] = h.hexdigest()
    return hashes


def digest(co):
    funcs, kernels = functions(co)
    res, code = resources(co), code_hashes(co)
    lines = []
    for name in sorted(funcs):
        r = ""
        if name in kernels:
            r = " ".join("%s=%s" % (k.strip(".").replace("_count", "").replace("_fixed_size", ""), res[name][k]) for k in KERNEL_KEYS)
        lines.append("%s size=%d %s code=%s" % (name, funcs[name], r or "(not a kernel)", code[name][:16]))
    total = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    lines.append("# %d kernels, %d FUNC symbols, sha256 of the lines above %s" % (len(kernels), len(funcs), total))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=os.path.join(CSRC, "bbme_device.hip"), help="the translation unit to compile")
    ap.add_argument("--code-object", help="an unbundled gfx950 code object to read instead of compiling")
    ap.add_argument("--out", help="write the digest here instead of standard output")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        text = digest(args.code_object or code_object(args.source, tmp))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
        print(text.splitlines()[-1])
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
