"""The table of coarse grids a speculative search may predict from (csrc/spec_grids.hpp, filled on the host and indexed by
k_search_fast): tests/cpp/spec_grids_test.cpp, a program of its own under AddressSanitizer and UBSan, reads through every entry
the cells the search kernel can ask for, for block sizes 2 .. 64, out of buffers of exactly the sizes the context allocates."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_table_entry_indexes_inside_its_buffer(tmp_path):
    exe = str(tmp_path / "spec_grids_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "spec_grids_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec grids ok" in r.stdout
