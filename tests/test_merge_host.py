"""CPU: the host side of sfmx_merge_pointcloud_3d2d (include/sfmx_scene.h) — exports, the defaults, the
n_new == 0 pass-through and the argument validation, none of which needs a device."""
import os
import subprocess

import numpy as np
import pytest

import sfmx
from sfmx import _lib, scene
import diag
import merge_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def known():
    return merge_cases.known_cases()["linked_near"][0]


def test_exported_by_product_and_diagnostic_library():
    for name in ("sfmx_merge_pointcloud_3d2d", "sfmx_merge_pointcloud_last_kernel_ms", "sfmx_merge_pointcloud_last_stats"):
        assert hasattr(_lib.lib, name) and hasattr(diag.diag_lib(), name) and name in _lib.PROTOTYPES, name
    assert sfmx.merge_pointcloud_3d2d is scene.merge_pointcloud_3d2d
    assert callable(scene.merge_pointcloud_3d2d_device) and callable(scene.merge_last_kernel_ms)


def test_header_defaults(tmp_path):
    src = tmp_path / "defaults.c"
    src.write_text('#include <stdio.h>\n#include "sfmx_scene.h"\n'
                   'int main(void){printf("%.17g %.17g\\n", SFMX_POINT_MERGE_DISTANCE, SFMX_FEATURE_MERGE_DISTANCE);return 0;}')
    exe = tmp_path / "defaults"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    d, f = map(float, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (d, f) == (scene.POINT_MERGE_DISTANCE, scene.FEATURE_MERGE_DISTANCE) == (0.01, 20.0)


def test_no_new_elements_pass_the_cloud_through_without_a_device(known):
    kps, pairs, m, off, cx, co, cs, cxy = known[:8]
    none = (np.zeros((0, 3)), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2)))
    r = scene.merge_pointcloud_3d2d(kps, pairs, m, off, cx, co, cs, cxy, *none)
    assert np.array_equal(r["xyz"], cx) and np.array_equal(r["origin_offsets"], co)
    assert np.array_equal(r["origin_shot"], cs) and np.array_equal(r["origin_xy"], cxy)
    assert r["target"].shape == (0,) and r["merge_distance"].shape == (0,) and scene.merge_last_kernel_ms() == 0.0
    assert scene.merge_last_stats() == dict(merged_static=0, merged_dynamic=0, links=0)
    r = scene.merge_pointcloud_3d2d(kps, pairs, m, off, *none, *none)
    assert r["xyz"].shape == (0, 3) and r["origin_offsets"].tolist() == [0] and r["origin_xy"].shape == (0, 2)


def test_argument_errors(known):
    kps, pairs, m, off, cx, co, cs, cxy, nx, no, ns, nxy, D, F = known
    call = scene.merge_pointcloud_3d2d
    nan = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        call(kps, pairs, m, off, cx, co, cs, cxy, nx, no, ns, nxy, nan, F)
    with pytest.raises(ValueError, match="NaN"):
        call(kps, pairs, m, off, cx, co, cs, cxy, nx, no, ns, nxy, D, nan)
    with pytest.raises(ValueError, match="cloud origin offsets"):
        call(kps, pairs, m, off, cx, np.array([0, 2, 1], np.int64), [0, 0], np.zeros((2, 2)), nx, no, ns, nxy)
    with pytest.raises(ValueError, match="cloud origin offsets"):
        call(kps, pairs, m, off, cx, co + 1, [0, 0, 0], np.zeros((3, 2)), nx, no, ns, nxy)
    with pytest.raises(ValueError, match="new origin offsets"):
        call(kps, pairs, m, off, cx, co, cs, cxy, np.zeros((2, 3)), np.array([0, 2, 1], np.int64), ns, nxy)
    with pytest.raises(ValueError, match="new origin offsets"):
        call(kps, pairs, m, off, cx, co, cs, cxy, nx, np.array([1, 2], np.int64), ns, nxy)
    with pytest.raises(ValueError, match="pair offsets"):
        call(kps, [[0, 1], [1, 2]], m, np.array([0, 5, 3], np.int64), cx, co, cs, cxy, nx, no, ns, nxy)
    with pytest.raises(ValueError, match="cloud origin shot"):
        call(kps, pairs, m, off, cx, co, [0, 4], cxy, nx, no, ns, nxy)
    with pytest.raises(ValueError, match="cloud origin shot"):
        call(kps, pairs, m, off, cx, co, [-1, 0], cxy, nx, no, ns, nxy)
    with pytest.raises(ValueError, match="new origin shot"):
        call(kps, pairs, m, off, cx, co, cs, cxy, nx, no, [1, 4], nxy)
    with pytest.raises(ValueError, match="pair shot"):
        call(kps, [[0, 4]], m, off, cx, co, cs, cxy, nx, no, ns, nxy)
    with pytest.raises(ValueError, match="pair shot"):
        call(kps, [[-1, 1]], m, off, cx, co, cs, cxy, nx, no, ns, nxy)
    # the errors are found before the device is looked for: also with nothing new to merge
    with pytest.raises(ValueError, match="NaN"):
        call(kps, pairs, m, off, cx, co, cs, cxy, np.zeros((0, 3)), [0], [], np.zeros((0, 2)), nan, F)


def test_point_count_beyond_int32_is_rejected():
    """n_cloud + n_new > INT32_MAX is refused from the counts alone (no array is read before that check)."""
    import ctypes as C
    z64 = np.zeros(2, np.int64)
    k, r = C.c_int32(0), C.c_int64(0)
    nkp = np.zeros(1, np.int32)
    ptrs = (C.c_void_p * 1)()
    rc = _lib.lib.sfmx_merge_pointcloud_3d2d(ptrs, nkp.ctypes.data_as(C.POINTER(C.c_int32)), 0, None, 0, None, None,
                                             None, 2 ** 31 - 1, z64.ctypes.data, None, None, None, 1, z64.ctypes.data,
                                             None, None, 0.01, 20.0, 0, 0, None, None, None, None, z64.ctypes.data, None, None,
                                             C.byref(k), C.byref(r))
    assert rc == _lib.SFMX_EINVAL and b"int32" in _lib.lib.sfmx_last_error()
