"""CPU: the -Prun=pcl-stats sub-program (PclStatsCli.cpp:30-79) as far as it goes without a device: the
flags and their defaults, the usage text, and the exits that happen before the search."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sfm-mvs-pipeline_amd"))

from sfmx import cli  # noqa: E402
import cloud_ref  # noqa: E402

EXE = os.path.join(REPO, "sfm-mvs-pipeline_amd", "bin", "Photogrammetrie")
RUN_SCRIPTS = json.load(open(os.path.join(REPO, "tests", "golden", "run_scripts.json")))


def run_exe(args, cwd=None):
    env = dict(os.environ, SFMX_NO_TORCH="1")
    return subprocess.run([sys.executable, EXE] + list(args), capture_output=True, text=True, cwd=cwd, env=env, timeout=120)


def test_usage_text():
    u = cli.usage("Photogrammetrie", 2)
    assert u.startswith("usage: Photogrammetrie -Prun=pcl-stats")
    for flag, default in (("-Pinput", "pointcloud.ply"), ("-Pstats", "optional"), ("-Pneighbors", "optional"),
                          ("-Pquality", "optional"), ("--help", "")):
        line = [l for l in u.splitlines() if l.strip().startswith(flag)]
        assert len(line) == 1 and default in line[0], flag
    assert "pcl-stats" in cli.usage("P", 0)
    assert cli.lib.sfmx_cli_usage(b"x", 3, None, 0) == -1


def test_flag_defaults():
    a = cli.AppArgs(["-Prun=pcl-stats"])
    assert a.getArg("input", "pointcloud.ply") == "pointcloud.ply"
    assert [a.getArg(k, "") for k in ("stats", "neighbors", "quality")] == ["", "", ""]
    c, _ = cli.configure(a)
    assert c.run == cli.RUN_PCL_STATS
    a = cli.AppArgs(RUN_SCRIPTS["run-pcl-stats.sh"][1:])
    assert a.getArg("run") == "pcl-stats" and a.getArg("input", "pointcloud.ply") != ""


def test_help_exits_255():
    r = run_exe(["-Prun=pcl-stats", "--help"])
    assert r.returncode == 255 and "-Pneighbors" in r.stdout and "-Pquality" in r.stdout and "EOL" not in r.stdout
    assert cli.PclStatsCli(cli.AppArgs(["--help"])).main() == 255


def test_missing_or_malformed_input_exits_255(tmp_path):
    """Deviation from the reference, which ignores loadPLYFile's result and goes on with an empty cloud."""
    r = run_exe(["-Prun=pcl-stats"], cwd=tmp_path)                  # the default input pointcloud.ply is not there
    assert r.returncode == 255 and "[ERROR]" in r.stdout and "pointcloud.ply" in r.stdout
    out = tmp_path / "stats.csv"
    r = run_exe(["-Prun=pcl-stats", "-Pinput=" + str(tmp_path / "nope.ply"), "-Pstats=" + str(out)])
    assert r.returncode == 255 and "nope.ply" in r.stdout and not out.exists()
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    r = run_exe(["-Prun=pcl-stats", "-Pinput=" + str(bad), "-Pstats=" + str(out)])
    assert r.returncode == 255 and "binary_big_endian" in r.stdout and not out.exists()


def test_sfmx_plan_has_no_plan_to_print(tmp_path):
    r = run_exe(["-Prun=pcl-stats", "--sfmx-plan"], cwd=tmp_path)
    assert r.returncode == 255 and "outside the sfmx hot path" in r.stdout
    argv = RUN_SCRIPTS["run-pcl-stats.sh"][1:] + ["--sfmx-plan"]
    r = run_exe(argv, cwd=tmp_path)
    assert r.returncode == 255 and "outside the sfmx hot path" in r.stdout


def test_cloud_of_one_point_needs_no_device(tmp_path):
    """n <= 1: the distance list is empty (the reference's size > 1 guard), nothing is launched, and the three
    files are those of the empty list."""
    ply = tmp_path / "one.ply"
    x = np.array([[1, 2, 3]], np.float32)
    cloud_ref.write_ply(str(ply), x, [3], [0, 0, 0])
    outs = [str(tmp_path / n) for n in ("s.csv", "n.csv", "q.ply")]
    r = run_exe(["-Prun=pcl-stats", "-Pinput=" + str(ply), "-Pstats=" + outs[0], "-Pneighbors=" + outs[1],
                 "-Pquality=" + outs[2]])
    assert r.returncode == 0 and "EOL" in r.stdout, r.stdout + r.stderr
    assert open(outs[0], "rb").read() == cloud_ref.stats_csv(cloud_ref.statistics([], 1))
    assert open(outs[1], "rb").read() == b"Distance,Count\n"
    assert open(outs[2], "rb").read() == cloud_ref.quality_ply(x, [], [3], [0, 0, 0])
