"""The wave-level model of k_reg_solve's schedule (tests/cpp/flood_model.cpp), a program of its own under AddressSanitizer and
UBSan (nothing is loaded into Python), linked with the oracle's C file: the instrument that prices flood speculation
(k_reg_solve<.., true>, BBME_FLOOD_RULE) and queue sharing before anything runs on a GPU.

On a small pair with a motion boundary it must
1. leave, in each of its four cases (plain, flood speculation, shared queues, both) and in every sweep of the pyramid, the
   field of the oracle's raster sweep, and
2. show a sweep at 8 x 8 blocks that needs at least 16 rounds of its busiest wave without speculation and fewer with it --
   the situation the kernel variant is built for."""
import os
import re
import subprocess

import pytest

import blockbasedmotionestimation_amd as bbme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 2 x 2 motion tiles of 256 x 192 pixels: floods of up to 32 blocks at 8 x 8 in a grid of 64 x 48
W, H, LEVELS, BLOCK, SEARCH, SEED, TILES, MOTION = 512, 384, 3, 16, 30, 20, 2, 20

SWEEP = re.compile(r"^sweep level=(\d+) b=(\d+) mult=(\d+) blocks=(\d+) rounds plain=(\d+) flood=(\d+) share=(\d+) both=(\d+) "
                   r"evaluated plain=(\d+) both=(\d+) speculated=(\d+) kept=(\d+) field=(\w+)$")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flood_model")
    exe, obj = str(tmp / "flood_model"), str(tmp / "bbme_oracle.o")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
    subprocess.check_call(["gcc", "-c", "-Wall"] + san + [os.path.join(ROOT, "oracle", "bbme_oracle.c"), "-o", obj])
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + san + ["-I", os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "flood_model.cpp"), obj, "-lm", "-o", exe])
    f1, f2, _ = bbme.synth_pair(W, H, SEED, max_motion=MOTION, tiles=TILES)
    paths = []
    for i, f in enumerate((f1, f2)):
        paths.append(str(tmp / ("frame%d.raw" % i)))
        f.tofile(paths[-1])
    r = subprocess.run([exe, str(W), str(H), str(LEVELS), str(BLOCK), str(SEARCH)] + paths, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flood model ok" in r.stdout
    rows = [SWEEP.match(line) for line in r.stdout.splitlines() if line.startswith("sweep ")]
    assert rows and all(rows), r.stdout
    keys = ("level", "b", "mult", "blocks", "plain", "flood", "share", "both", "evaluated", "evaluated_both", "speculated", "kept")
    return [dict(zip(keys, map(int, m.groups()[:-1])), field=m.group(13)) for m in rows]


def test_every_modelled_field_is_the_raster_sweeps(table):
    # three levels, block sizes 16 .. 2, two sweeps each
    assert len(table) == LEVELS * 4 * 2
    assert all(row["field"] == "same" for row in table), table


def test_a_sweep_at_8x8_is_a_chain_that_speculation_shortens(table):
    rows = [row for row in table if row["b"] == 8]
    assert len(rows) == LEVELS * 2
    deep = [row for row in rows if row["plain"] >= 16]
    assert deep, rows
    # fewer with it: on its own, and on top of the shared queues the kernel runs with; and not vacuously -- evaluations were
    # made on speculation, and some of them counted
    assert any(row["flood"] < row["plain"] and row["both"] < row["share"] and row["kept"] > 0 for row in deep), deep
