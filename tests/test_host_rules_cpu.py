"""The CPU rules of csrc/bbme_host.cpp -- consistency, interpolation (grey and B,G,R), the temporal filters, subpel, motion
compensation: the references the GPU tests compare against -- under AddressSanitizer and UBSan, as a program of its own
(tests/cpp/host_rules_test.cpp and bbme_host.cpp, nothing loaded into Python): exactly sized outputs, vectors on and one past the
last legal position, every legal and illegal kind of window, and the grey temporal filter against the colour one on B = G = R."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_rules_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "host_rules_test.cpp"),
                           os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc", "bbme_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host rules ok" in r.stdout
