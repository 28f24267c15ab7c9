"""The five host calls of the global motion rule and the global compensation rule of csrc/bbme_host.cpp -- the references the GPU
tests of K16 - K18 compare against -- under AddressSanitizer and UBSan, as a program of its own
(tests/cpp/global_motion_host_test.cpp and bbme_host.cpp, nothing loaded into Python): exactly sized grids, masks, planes and
outputs, int16-extreme grids, int32-extreme models, tolerances 0 and 2^40, every kind of window."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_global_motion_host_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "global_motion_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "global_motion_host_test.cpp"),
                           os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc", "bbme_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "global motion host rules ok" in r.stdout
