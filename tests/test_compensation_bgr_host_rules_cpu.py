"""The host call of the BGR compensation rule of csrc/bbme_host.cpp -- the reference the GPU tests of K11b compare against -- under
AddressSanitizer and UBSan, as a program of its own (tests/cpp/compensation_bgr_host_test.cpp and bbme_host.cpp, nothing loaded
into Python): frames, grids and outputs allocated to the exact size at odd pads and pitches, the edge and extreme grids in both
units, every kind of window, and B = G = R frames against the grey rules on the padded plane."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compensation_bgr_host_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "compensation_bgr_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "compensation_bgr_host_test.cpp"),
                           os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc", "bbme_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compensation bgr host rule ok" in r.stdout
