"""GPU: -Prun=pcl-stats end to end on the golden mesh written as a PLY file: one search, three files, each equal to
the numpy restatement's bytes (tests/cloud_ref.py)."""
import numpy as np
import pytest

import cloud_ref
import fixtures
from sfmx import cli

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
def test_pcl_stats_writes_the_three_files(binary, tmp_path):
    g = fixtures.load("cloud_small")
    x, fs, fi = g["xyz"], g["face_sizes"].tolist(), g["face_indices"].tolist()
    at = int(np.sum(fs[:fs.index(256)]))
    fs, fi = fs[:fs.index(256)] + fs[fs.index(256) + 1:], fi[:at] + fi[at + 256:]      # a PLY list holds at most 255
    ply = str(tmp_path / "mesh.ply")
    cloud_ref.write_ply(ply, x, fs, fi, binary=binary, vertex_extra=[("uchar", "red", 9)])
    outs = [str(tmp_path / n) for n in ("stats.csv", "neighbors.csv", "quality.ply")]
    rc = cli.main(["Photogrammetrie", "-Prun=pcl-stats", "-Pinput=" + ply, "-Pstats=" + outs[0], "-Pneighbors=" + outs[1],
                   "-Pquality=" + outs[2]])
    assert rc == 0
    d = g["distance"]
    assert open(outs[0], "rb").read() == g["stats_csv"].tobytes()
    assert open(outs[1], "rb").read() == g["neighbors_csv"].tobytes()
    assert open(outs[2], "rb").read() == cloud_ref.quality_ply(x, d, fs, fi)
    # only the statistics: the other files are not written
    only = str(tmp_path / "only.csv")
    assert cli.main(["Photogrammetrie", "-Prun=pcl-stats", "-Pinput=" + ply, "-Pstats=" + only]) == 0
    assert open(only, "rb").read() == g["stats_csv"].tobytes()
