"""CPU: the host side of sfmx_triangulate_matches (include/sfmx_triangulate.h) — exports, struct layout,
argument validation and the empty calls, none of which needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sfmx import _lib, triangulate
import diag
import tri_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return tri_cases.small_case()


def test_exported_by_product_and_diagnostic_library():
    for name in ("sfmx_triangulate_matches", "sfmx_triangulate_last_kernel_ms"):
        assert hasattr(_lib.lib, name) and hasattr(diag.diag_lib(), name), name
    import sfmx
    assert sfmx.triangulateMatch is triangulate.triangulateMatch and sfmx.triangulate_matches is triangulate.triangulate_matches


def test_camera_struct_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfmx_triangulate.h"\n'
                   'int main(void){printf("%zu %zu %zu %g\\n", sizeof(sfmx_tri_camera), offsetof(sfmx_tri_camera, K),'
                   ' offsetof(sfmx_tri_camera, dist), SFMX_MAX_REPROJECTION_ERROR);return 0;}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    size, k, d, mx = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    S = _lib.sfmx_tri_camera
    assert (int(size), int(k), int(d)) == (C.sizeof(S), S.K.offset, S.dist.offset) == (112, 0, 72)
    assert float(mx) == triangulate.MAX_REPROJECTION_ERROR == 10.0


def test_empty_calls_need_no_device(case):
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    for prs in (np.zeros((0, 2), np.int32), pairs[:7]):
        r = triangulate.triangulate_matches(kps, cams, sc, poses, prs, m[:0], np.zeros(len(prs) + 1, np.int64))
        assert r["n_points"] == 0 and r["point_offsets"].tolist() == [0] * (len(prs) + 1)
        assert r["xyz"].shape == (0, 3) and r["match"].shape == (0,) and r["origin_xy"].shape == (0, 2)
        assert r["origin_offsets"].tolist() == [0] and r["err"].shape == (0, 2)
        assert triangulate.last_kernel_ms() == 0.0


def test_argument_errors(case):
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    z = np.zeros(4, np.int64)
    with pytest.raises(ValueError, match="camera index"):
        triangulate.triangulate_matches(kps, cams, [0, 1, 2, 1, 0, 1], poses, pairs[:3], m[:0], z)
    with pytest.raises(ValueError, match="camera index"):
        triangulate.triangulate_matches(kps, cams, [0, 1, -1, 1, 0, 1], poses, pairs[:3], m[:0], z)
    for K in (np.array([0.0, 0, 1, 0, 5, 1, 0, 0, 1]), np.array([5.0, 0, 1, 0, 0, 1, 0, 0, 1])):
        with pytest.raises(ValueError, match="focal"):
            triangulate.triangulate_matches(kps, [cams[0], (K, np.zeros(5))], sc, poses, pairs[:3], m[:0], z)
    with pytest.raises(ValueError, match="pair shot"):
        triangulate.triangulate_matches(kps, cams, sc, poses, [[0, 6]], m[:0], np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="ascending"):
        triangulate.triangulate_matches(kps, cams, sc, poses, pairs[:3], m[:0], np.array([0, 2, 1, 0], np.int64))
    with pytest.raises(ValueError, match="start at 0"):
        triangulate.triangulate_matches(kps, cams, sc, poses, pairs[:3], m[:0], np.array([1, 1, 1, 0], np.int64))
    with pytest.raises(ValueError):
        triangulate.triangulate_matches(kps, cams, sc, poses, pairs[:3], m[:5], z)             # offsets do not cover the list
    with pytest.raises(ValueError):
        triangulate.triangulate_matches(kps, cams, sc[:5], poses, pairs[:3], m[:0], z)         # one camera index per shot
