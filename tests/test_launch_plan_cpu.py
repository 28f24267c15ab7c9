"""The launch plan of an estimate (csrc/launch_plan.hpp) without a GPU: tests/cpp/launch_plan_test.cpp, a program of its own under
AddressSanitizer and UBSan (nothing is loaded into Python), linked with bbme_host.cpp for the real level sizes and two-wave verdicts.

1. Its invariants over block sizes 2 .. 64, one to four levels, single / batched / chain pair counts, both regulariser and search
   modes, speculation on and off and every knob at the values the GPU tests use.
2. Its dump (one line per kernel launch) for every case the GPU tests use to reach a form: the form must be in the plan, so a
   geometry that silently misses a knob's conditions fails here instead of passing bit-exactly on another kernel.
3. Its dump for bench.py's workloads against tests/golden/launch_plans.txt: a change of the launch sequence is a diff of that file.

What the dump cannot show, and why -- these cases are only checked to plan the kernel the knob acts in:
  BBME_LOCAL_ROUNDS    a kernel argument of k_reg_iter (the plan must launch k_reg_iter)
  BBME_LOOSE_PLAN      another task table for the same k_search_fast launch (the plan must launch k_search_fast)
  BBME_MEMO_FORWARD    a kernel argument of the memo solver (the plan must launch it)
  BBME_NO_GRAPH        how the same plan is enqueued (eagerly instead of captured): the plan is the default's
  BBME_SOLVE_SHARE, BBME_WIDE_THRESHOLD, BBME_TEST_ROUND_CAP    kernel arguments of k_reg_solve"""
import os
import re
import subprocess

import pytest

import helpers as H
from test_gpu_context_state import GEOMETRIES
from test_gpu_spec_late import BATCH_SEEDS, CASES as LATE_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blockbasedmotionestimation_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_plans.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "launch_plan_test.cpp"), os.path.join(CSRC, "bbme_host.cpp"), "-o", path])
    return path


def test_invariants_under_sanitizers(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "launch plan ok" in r.stdout


LAUNCH = re.compile(r"^(\w+)(?:<([^>]*)>)? grid=(\d+)x(\d+) wg=(\d+) lds=(\d+) stream=(main|side)$")


class Plan:
    """The dump: `launches` [(kernel, template arguments, grid x, grid y, workgroup, LDS, stream)], `notes` (the '#' lines)."""

    def __init__(self, text):
        self.text = text
        self.notes = [line for line in text.splitlines() if line.startswith("#")]
        self.launches = []
        for line in text.splitlines():
            m = LAUNCH.match(line)
            if m:
                k, targs, gx, gy, wg, lds, stream = m.groups()
                self.launches.append((k, tuple(targs.split(", ")) if targs else (), int(gx), int(gy), int(wg), int(lds), stream))
            else:
                assert line.startswith("#"), line

    def of(self, kernel, **where):
        """launches of `kernel`; b=: first template argument; last=: last template argument"""
        out = [l for l in self.launches if l[0] == kernel]
        if "b" in where:
            out = [l for l in out if l[1][0] == str(where["b"])]
        if "last" in where:
            out = [l for l in out if l[1][-1] == str(where["last"])]
        return out

    def sweeps(self):
        return [n for n in self.notes if " sweep b=" in n]


def dump(exe, w, h, search, block, env=None, **opts):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BBME_")}
    cmd = [exe, "dump", str(w), str(h), ",".join(map(str, search)), ",".join(map(str, block))] + ["%s=%d" % kv for kv in opts.items()]
    r = subprocess.run(cmd, env=dict(clean, **(env or {})), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return Plan(r.stdout)


# ---- the result-neutral knobs (helpers.KNOB_CASES): what the plan of every geometry must show under the knob -------------------
def _knob_form(name, plan, default):
    """None, or what is missing.  `default`: the plan of the same geometry with the knob's own variable at its default."""
    if name == "list_split":                        # two waves per listed block without the knob, one with it
        if not default.of("k_search_list", last=2):
            return "no two-wave fix-up list to take away: %s" % sorted(set(l[:2] for l in default.of("k_search_list")))
        return None if plan.of("k_search_list") and not plan.of("k_search_list", last=2) else "a two-wave list is left"
    if name == "pass1_eager":                       # a lazy pass 1 in front of the forced relaxation launch without the knob
        if not any("lazy=1" in n for n in default.sweeps()):
            return "no sweep is lazy under BBME_RELAX_STEPS=1 alone: pass 1 has the chain form on every grid"
        return None if not any("lazy=1" in n for n in plan.sweeps()) and plan.of("k_reg_iter") else "a lazy sweep is left"
    if name == "xcd_natural":                       # a k_search_fast grid that the XCD-aware order would pad
        return None if any(l[2] % 8 for l in plan.of("k_search_fast")) else "every k_search_fast grid is a multiple of 8"
    if name.startswith("loose_plan"):
        return None if plan.of("k_search_fast") else "no k_search_fast launch"
    if name == "relax_rule":                        # two relaxation launches in front of both sweeps, on every grid
        return None if len(plan.of("k_reg_iter")) == 2 * len(plan.sweeps()) else "%d k_reg_iter launches for %d sweeps" % (
            len(plan.of("k_reg_iter")), len(plan.sweeps()))
    if name.startswith("local_rounds"):
        return None if len(plan.of("k_reg_iter")) == len(plan.sweeps()) else "not one k_reg_iter launch per sweep"
    if name == "no_graph":
        return None if plan.text == default.text else "BBME_NO_GRAPH changes the plan"
    return "no form is written down for this knob"


# the variable whose default the knob's plan is compared with (the others of the case's environment stay)
_KNOB_OWN = {"list_split": "BBME_LIST_SPLIT", "pass1_eager": "BBME_PASS1_LAZY", "no_graph": "BBME_NO_GRAPH"}
# Geometries found NOT to reach the form they were written for; they stay in the GPU test (their fields are still checked), and a
# geometry that does reach it stands beside them in the case.  pass1_eager: pass 1 is lazy only in the strip form, which a single
# pair takes only where the chain form does not (more than BBME_PASS1_LANES_MAX = 140 000 blocks): both 2 x 2 grids here are
# smaller (22 528 and 12 288 blocks), so BBME_PASS1_LAZY=0 changed nothing in them.
KNOWN_MISSES = {("pass1_eager", (352, 256)), ("pass1_eager", (256, 192))}


@pytest.mark.parametrize("name,env,cases", H.KNOB_CASES, ids=[k[0] for k in H.KNOB_CASES])
def test_knob_cases_reach_their_form(exe, name, env, cases):
    reached = 0
    for w, h, search, block, _ in cases:
        plan = dump(exe, w, h, search, block, env)
        default = dump(exe, w, h, search, block, {k: v for k, v in env.items() if k != _KNOB_OWN.get(name)})
        missing = _knob_form(name, plan, default)
        if (name, (w, h)) in KNOWN_MISSES:
            assert missing is not None, "%s on %s reaches its form after all: take it off KNOWN_MISSES" % (name, (w, h, search, block))
        else:
            assert missing is None, "%s on %s: %s" % (name, (w, h, search, block), missing)
            reached += 1
    assert reached, "%s: no geometry reaches the form" % name


# ---- the regulariser's forms (helpers.LIMIT_REG_FORMS) on the limit contents; the stage calls plan every sweep as an estimate does ----
def _reg_form(form, plan, block, levels):
    bs = [b for b in (64, 32, 16, 8, 4, 2) if b <= block]
    solves = plan.of("k_reg_solve")
    if form == "pass1_strip":
        return all(plan.of("k_reg_pass1_strip", b=b) for b in (4, 2)) and not plan.of("k_reg_pass1_lanes")
    if form == "pass1_lanes_low":
        return all(len(plan.of("k_reg_pass1", b=b)) == 2 * levels for b in bs) and not plan.of("k_reg_pass1_lanes") and not plan.of("k_reg_pass1_strip")
    if form == "pass1_lanes_high":
        return all(len(plan.of("k_reg_pass1_lanes", b=b)) == 2 * levels for b in bs if b <= 16)
    if form == "solve_waves_1":
        return solves and all(l[4] == 64 for l in solves)
    if form == "solve_one_wave":
        return solves and all(l[4] == 64 and l[2] == 8 for l in solves)     # (one share per XCD: eight workgroups, seven of them idle)
    if form == "relax_rule":
        return all(len(plan.of("k_reg_iter", b=b)) == 3 * levels for b in bs)        # two in front of the first sweep, one of the second
    if form == "memo_off":
        return not plan.of("k_reg_pass1_lanes", last="true") and not plan.of("k_reg_solve", last="true")
    if form in ("memo_b8", "memo_b8_forward"):
        return all(len(plan.of("k_reg_pass1_lanes", b=b, last="true")) == 2 * levels and len(plan.of("k_reg_solve", b=b, last="true")) == 2 * levels
                   for b in bs if b >= 8) and not any(plan.of("k_reg_solve", b=b, last="true") for b in (4, 2))
    raise AssertionError("no form is written down for " + form)


@pytest.mark.parametrize("form", list(H.LIMIT_REG_FORMS))
@pytest.mark.parametrize("name", H.LIMIT_REG_CONTENTS)
def test_regulariser_forms_are_planned(exe, name, form):
    c = H.LIMIT_CONTENTS[name]
    plan = dump(exe, c["w"], c["h"], c["search"], c["block"], H.LIMIT_REG_FORMS[form], raster=int(c["raster"]), speculate=0)
    assert _reg_form(form, plan, max(c["block"]), len(c["block"])), "%s on %s:\n%s" % (form, name, plan.text)


# ---- the search forms of helpers.LIMIT_SEARCH_CASES that an environment selects ---------------------------------------------------
def _search_groups():
    for name, env in H.LIMIT_SEARCH_CASES:
        if env == H._SPLIT_ON:
            yield name, env, "two_waves"
        elif "BBME_LOOSE_PLAN" in env:
            yield name, env, "loose"
        elif "BBME_GENERIC_SEARCH" in env:
            yield name, env, "generic"


@pytest.mark.parametrize("name,env,form", list(_search_groups()), ids=["%s-%s" % (n, f) for n, _, f in _search_groups()])
def test_search_forms_are_planned(exe, name, env, form):
    c = H.LIMIT_CONTENTS[name]
    plan = dump(exe, c["w"], c["h"], c["search"], c["block"], env, raster=int(c["raster"]), speculate=0)
    levels = len(c["block"])
    if form == "two_waves":
        assert len(plan.of("k_search_fast", last=2)) == levels and not plan.of("k_search_generic"), plan.text
    elif form == "loose":
        assert len(plan.of("k_search_fast", last=1)) == levels, plan.text
    else:
        assert len(plan.of("k_search_generic")) == levels and not plan.of("k_search_fast"), plan.text


# ---- the speculative search's late predictions (test_gpu_spec_late) -----------------------------------------------------------------
def _forks(plan):
    """[(level searched, the sweep note in front of the fork, late, late_force)]"""
    out = []
    for i, n in enumerate(plan.notes):
        m = re.match(r"# level (\d+) fork, speculative search late=(\d) late_force=(\d)", n)
        if m:
            out.append((int(m.group(1)), plan.notes[i - 1], int(m.group(2)), int(m.group(3))))
    return out


@pytest.mark.parametrize("late", (0, 1, 2))
@pytest.mark.parametrize("fork_first", (None, 0, 1))
@pytest.mark.parametrize("pairs", (1, len(BATCH_SEEDS)))
@pytest.mark.parametrize("name", list(LATE_CASES))
def test_late_prediction_cases_fork_where_they_say(exe, name, pairs, fork_first, late):
    w, h, _, _, search, block = LATE_CASES[name]
    env = {"BBME_SPEC_MIN_GABS": "0", "BBME_SPEC_LATE": str(late)}
    if fork_first is not None:
        env["BBME_SPEC_FORK_FIRST"] = str(fork_first)
    plan = dump(exe, w, h, search, block, env, pairs=pairs)
    forks = _forks(plan)
    assert [f[0] for f in forks] == list(range(len(block) - 2, -1, -1)), "every level but the coarsest is speculated\n" + plan.text
    assert plan.notes[-1] == "# speculated levels mask %d" % (2 ** (len(block) - 1) - 1)
    behind_first = late != 0 and fork_first != 0
    for level, sweep, is_late, force in forks:
        assert "sweep b=%d mult=%d " % (block[level + 1], 1 if behind_first else 2) in sweep, (level, sweep)
        assert (is_late, force) == (int(late != 0), int(late == 2)), (level, is_late, force)
        assert ("publish=0" in sweep) == (late != 0), sweep
    published = [int(n.rsplit("publish=", 1)[1]) for n in plan.sweeps() if "publish=-1" not in n]
    assert bool(published) == (late != 0) and all(g == pairs for l in plan.launches for g in [l[3]])
    assert len(plan.of("k_search_list")) == len(block) - 1 and len(plan.of("k_fixup_list")) == len(block) - 1


# ---- the LDS floor of the speculative launches (test_gpu_context_state.test_speculative_search_lds_floor) ------------------------------
@pytest.mark.parametrize("per_cu", ["2", "1", "24,1"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_lds_floor_is_in_the_speculative_launches(exe, geom, per_cu):
    w, h, search, block = GEOMETRIES[geom]
    plan = dump(exe, w, h, search, block, {"BBME_SPEC_WGS_PER_CU": per_cu, "BBME_SPEC_MIN_GABS": "0"})
    side = [l for l in plan.launches if l[6] == "side"]
    assert [f[0] for f in _forks(plan)] == list(range(len(block) - 2, -1, -1)) and len(side) == len(block) - 1, plan.text
    floors = {"2": [61440] * 2, "1": [122880] * 2, "24,1": [5120, 122880]}[per_cu]       # 120 KB / n in units of 256 bytes; level 1, level 0
    for launch, floor in zip(side, floors):
        assert launch[5] >= floor and (launch[5] == floor or floor == 5120), (launch, floor)
    assert max(l[5] for l in plan.launches if l[6] == "main") < 48 * 1024 or geom == "generic"


# ---- bench.py's workloads against the committed plans ----------------------------------------------------------------------------
FIXTURE_WORKLOADS = [("cfg3", 1), ("cfg4", 1), ("cfg2", 1), ("cfg1", 1), ("ref", 1), ("cfg3", 6)]
_BENCH = {"cfg3": (3840, 2160, 80, 16, 4), "cfg2": (1920, 1080, 48, 16, 3), "cfg4": (3840, 2160, 72, 8, 4), "cfg1": (584, 388, 30, 16, 3),
          "ref": (2336, 1552, 64, 32, 4)}                # bench.py's WORKLOADS: width, height, search size, block size, levels


def fixture_text(exe):
    out = []
    for name, pairs in FIXTURE_WORKLOADS:
        w, h, search, block, levels = _BENCH[name]
        out.append("== %s, %s, default knobs ==\n" % (name, "single pair" if pairs == 1 else "batch of %d" % pairs))
        out.append(dump(exe, w, h, [search] * levels, [block] * levels, pairs=pairs).text)
    return "".join(out)


def test_bench_workloads_match_the_committed_plans(exe):
    committed = [line for line in open(FIXTURE).read().splitlines() if not line.startswith("##")]      # '##': the file's header
    assert fixture_text(exe).splitlines() == committed, "the launch sequence of a bench.py workload changed: see tests/golden/launch_plans.txt"
