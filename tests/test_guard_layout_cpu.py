"""The layout of a guarded device allocation (csrc/guard_layout.hpp) without a GPU: tests/cpp/guard_layout_test.cpp, a program of
its own under AddressSanitizer and UBSan (nothing is loaded into Python).  Offsets and alignment for payloads of 0, 1, 4095, 4096,
4097 and 8 294 400 bytes, the scan of a guard band's host copy with damage at its first byte, its last byte and on both sides,
a clean scan of an undamaged copy, and the parsing of BBME_TEST_GUARD / BBME_TEST_POISON.  tests/test_gpu_guards.py runs the
kernels between such guards."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("guard_layout") / "guard_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "guard_layout_test.cpp"),
                           "-o", path])
    return path


def test_layout_scan_and_knobs_under_sanitizers(exe):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BBME_")}
    r = subprocess.run([exe], env=clean, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "guard layout ok" in r.stdout


def test_hooks_are_declared_and_bound():
    """The three entry points are in include/bbme.h under the "test hooks" heading and in the ctypes table."""
    from blockbasedmotionestimation_amd import _capi
    header = open(os.path.join(ROOT, "include", "bbme.h")).read()
    hooks = header[header.index("test hooks"):]
    for name in ("bbme_test_guard_check", "bbme_test_guard_reset", "bbme_test_guard_find"):
        assert "int %s(" % name in hooks
        assert name in _capi.SIGNATURES
