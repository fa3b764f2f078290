"""CPU: the merge's path controls (include/sfmx_scene.h) — sfmx_merge_pointcloud_set_max_rounds and
sfmx_merge_pointcloud_last_path are exported by both libraries, take their arguments and answer before any
merge call, none of which needs a device."""
import ctypes as C
import threading

from sfmx import _lib, scene
import diag

NAMES = ("sfmx_merge_pointcloud_set_max_rounds", "sfmx_merge_pointcloud_last_path")


def test_exported_by_product_and_diagnostic_library():
    for name in NAMES:
        assert hasattr(_lib.lib, name) and hasattr(diag.diag_lib(), name) and name in _lib.PROTOTYPES, name
    assert callable(scene.merge_set_max_rounds) and callable(scene.merge_last_path)


def test_set_max_rounds_accepts_every_kind_of_value():
    try:
        for lib in (_lib.lib, diag.diag_lib()):
            for v in (-1, 0, 8):
                assert lib.sfmx_merge_pointcloud_set_max_rounds(v) == _lib.SFMX_OK
        for v in (-1, 0, 8):
            assert scene.merge_set_max_rounds(v) is None
    finally:
        scene.merge_set_max_rounds(0)


def test_last_path_before_any_call_is_zero():
    """The record is per thread: a thread that never merged reads zeros, whatever other threads did."""
    seen = {}

    def fresh():
        seen["mirror"] = scene.merge_last_path()
        r, f, b = C.c_int32(7), C.c_int32(7), C.c_int64(7)
        seen["rc"] = _lib.lib.sfmx_merge_pointcloud_last_path(C.byref(r), C.byref(f), C.byref(b))
        seen["raw"] = (r.value, f.value, b.value)
        seen["null"] = _lib.lib.sfmx_merge_pointcloud_last_path(None, None, None)

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen["mirror"] == dict(rounds=0, host_fallback=0, host_bytes=0)
    assert seen["rc"] == _lib.SFMX_OK and seen["raw"] == (0, 0, 0) and seen["null"] == _lib.SFMX_OK
