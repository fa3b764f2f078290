"""CPU: the planner and the graph checks of csrc/scene_plan.hpp under AddressSanitizer and UndefinedBehaviorSanitizer.

A stand-alone program (tests/cpp/scene_plan_main.cpp, its own main) includes only that header.  It checks the tables
that sfmx_find_3d2d_matches (one candidate) and sfmx_count_3d2d_matches (any candidates, a pair mask) plan, and the
first-pair flags of sfmx_merge_pointcloud_3d2d, against a brute-force restatement written in the program: per
(candidate, other shot) the lowest-index visible pair joining them in either orientation, dropped if its list is
empty.  Graphs: no pairs, a pair of a shot with itself, two shots joined in both orientations, a mask hiding the
first pair, an empty first pair before a non-empty duplicate (which must not be used), a candidate without a pair;
one candidate and all shots.  Then the table capacity at 0, 1, 8, 9 and 2^29 entries and every graph check's accept
and reject cases.  It runs as a child process and must exit clean.  The sanitizer runtimes are linked into the
program, so it needs nothing from the environment it is started in.  Fails without the feature: the header does not
exist."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_planner_under_sanitizers(tmp_path):
    exe = tmp_path / "scene_plan_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    os.path.join(REPO, "tests", "cpp", "scene_plan_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
    assert r.stdout == "ok 78\n"
