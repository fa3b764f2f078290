"""CPU: the argument errors of sfmx_find_3d2d_matches (include/sfmx_scene.h) that are found before a device is looked
for, as in sfmx_count_3d2d_matches: a shot or a pair shot out of range, a negative keypoint count, null origin arrays."""
import ctypes as C

import numpy as np
import pytest

from sfmx import _lib, scene
import scene_cases


def test_argument_errors_need_no_device():
    kps, pairs, m, off, oo, osh, oxy = scene_cases.edge_case()
    for shot in (-1, 4):
        with pytest.raises(ValueError, match="shot index"):
            scene.find_3d2d_matches(kps, pairs, m, off, oo, osh, oxy, shot)
    for bad in (-1, 4):
        bp = pairs.copy()
        bp[4, 0] = bad
        with pytest.raises(ValueError, match="pair shot"):
            scene.find_3d2d_matches(kps, bp, m, off, oo, osh, oxy, 0)


def test_negative_keypoint_count_and_null_origin_arrays():
    kps, pairs, m, off, oo, osh, oxy = scene_cases.edge_case()
    ptrs = (C.c_void_p * 4)(*[k.ctypes.data for k in kps])
    out = np.zeros(len(osh), np.int32)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def call(nkp, shot_ptr, xy_ptr):
        return _lib.lib.sfmx_find_3d2d_matches(ptrs, p32(nkp), 4, p32(pairs), len(pairs), m.ctypes.data, off.ctypes.data,
                                               oo.ctypes.data, len(oo) - 1, shot_ptr, xy_ptr, 0, 0, 0, None, out.ctypes.data,
                                               out.ctypes.data, None)
    assert call(np.array([12, 12, -1, 12], np.int32), osh.ctypes.data, oxy.ctypes.data) == _lib.SFMX_EINVAL
    assert b"negative keypoint count" in _lib.lib.sfmx_last_error()
    assert call(np.array([12, 12, 12, 12], np.int32), None, oxy.ctypes.data) == _lib.SFMX_EINVAL
    assert b"null origin arrays" in _lib.lib.sfmx_last_error()
