"""CPU: csrc/sfm_host.hpp under AddressSanitizer and UndefinedBehaviorSanitizer.

A stand-alone program (tests/cpp/sfm_host_main.cpp, its own main) includes the header, reads a scenario and the
answers every step gave in a tests/sfm_ref.py run over the toy world, answers each step call with the next
record and prints the trace.  It runs as a child process, must exit clean with nothing on stderr, and its trace
and outputs must equal the literal loop's.  The sanitizer runtimes are linked into the program, so it needs
nothing from the environment it is started in.  Fails without the feature: the header does not exist."""
import os
import subprocess

import numpy as np
import pytest

import sfm_ref
import sfm_toy
from sfmx import sfm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
KIND = {n: i for i, n in enumerate(sfm.STEP_NAMES)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sfm_host") / "sfm_host_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror",
                    os.path.join(REPO, "tests", "cpp", "sfm_host_main.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def scenario_text(sc, log):
    p = sc.params
    lines = [f"{sc.n_shots} {len(sc.pairs)} {p['min_match_count_for_baseline']} {p['min_homography_inlier_ratio']!r} "
             f"{p['min_pose_inlier_ratio']!r}"]
    lines += [f"{l} {r} {n} {float(h)!r}" for (l, r), n, h in zip(sc.pairs, sc.n_matches, sc.homography)]
    lines.append(str(len(log)))
    for e in log:
        k = KIND[e[0]]
        if e[0] == "count_candidates":
            body = [len(e[1]), *e[1], *e[2]]
        elif e[0] == "register_shot":
            body = [e[1], e[2], repr(float(e[3])), len(e[4]), *e[4]]
        else:
            body = list(e[1:])
        lines.append(" ".join(str(x) for x in [k, *body]))
    return "\n".join(lines) + "\n"


def replay(driver, tmp_path, sc):
    world = sfm_toy.World(sc)
    ref = sfm_ref.triangulate(world, sc.n_shots, sc.pairs, sc.n_matches, sc.homography, **sc.params)
    src = tmp_path / f"{sc.name}.txt"
    src.write_text(scenario_text(sc, world.log))
    r = subprocess.run([driver, str(src)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and r.stderr == "", (sc.name, r.stdout[-2000:] + r.stderr[-4000:])
    out = r.stdout.split("\n")
    assert out[0] == f"rc 0 events {len(ref['trace'])} replayed {len(world.log)} of {len(world.log)}", (sc.name, out[0])
    got = [l.split() for l in out if l.startswith("E ")]
    exp = [[str(sfm.EVENTS[e[0]]), str(e[1]), str(e[2]), np.float64(e[3]).tobytes()[::-1].hex()] for e in ref["trace"]]
    assert [g[1:] for g in got] == exp, sc.name
    row = lambda tag: next(l for l in out if l.startswith(tag)).split()[1:]
    assert row("R") == [str(int(v)) for v in ref["recovered"]], sc.name
    assert row("S") == [str(v) for v in ref["pair_state"]], sc.name
    assert row("C") == [str(v) for v in ref["pair_n_matches"]], sc.name
    assert row("B ")[:3] == [str(ref["ba"][k]) for k in ("calls", "iterations", "last")], sc.name
    if len(ref["trace"]) > 1:
        assert row("short") == [str(-4), "1"], sc.name


def test_named_scenes_under_sanitizers(driver, tmp_path):
    for sc in sfm_toy.named_scenarios():
        replay(driver, tmp_path, sc)


def test_random_graphs_under_sanitizers(driver, tmp_path):
    for sc in sfm_toy.random_scenarios(40):
        replay(driver, tmp_path, sc)


def test_invalid_arguments_under_sanitizers(driver, tmp_path):
    base = next(sc for sc in sfm_toy.named_scenarios() if sc.name == "ring6")
    for name, change in (("baseline3", dict(params=dict(min_match_count_for_baseline=3))),
                         ("ratio", dict(params=dict(min_pose_inlier_ratio=1.5))),
                         ("shot", dict(pairs=[(0, 6)] + [(1, 2)] * 5)),
                         ("count", dict(n_matches=[-1] + [200] * 5))):
        kw = dict(n_shots=6, pairs=base.pairs, n_matches=base.n_matches, homography=base.homography, pose=base.pose,
                  weight=base.weight, registration=base.registration)
        kw.update(change)
        sc = sfm_toy.Scenario(name, **kw)
        src = tmp_path / f"{name}.txt"
        src.write_text(scenario_text(sc, []))
        r = subprocess.run([driver, str(src)], capture_output=True, text=True, env=ENV)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("EINVAL "), (name, r.stdout + r.stderr)
