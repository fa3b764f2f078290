"""The diagnostic library in tests (test infrastructure).

lib/libsfmx.so reads no environment variable: its kernels are the shipped forms
only.  The kernel variants, the alternative BA factorization forms and the
timing probes live in lib/libsfmx_diag.so (`make diag`, -DSFMX_DIAG,
csrc/diag.hpp), which reads SFMX_SIFT_VARIANT, SFMX_SIFT_P2, SFMX_ORB_VARIANT,
SFMX_BA_ORDER / _BACK / _SPLIT / _DAG / _SPEC, SFMX_SIFT_SMALL[_PX],
SFMX_SIFT_XCD[_EXTREMA], SFMX_SIFT_EX_ROWS.

`diagnostic(**env)` loads that library next to the product one (both are
RTLD_LOCAL, so each resolves its own symbols and registers its own kernels),
points every sfmx module's `lib` at it and sets the variables for the block.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys

from sfmx import _lib

DIAG_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libsfmx_diag.so")
_diag = None


def diag_lib() -> C.CDLL:
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_PATH):
            raise ImportError(f"{DIAG_PATH} missing: build it with `make -C sfm-mvs-pipeline_amd diag`")
        lib = C.CDLL(DIAG_PATH)
        for name, (res, args) in _lib.PROTOTYPES.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        _diag = lib
    return _diag


@contextlib.contextmanager
def diagnostic(**env):
    """Run the block on lib/libsfmx_diag.so with the given tuning variables set."""
    dl = diag_lib()
    mods = [m for n, m in list(sys.modules.items())
            if (n == "sfmx" or n.startswith("sfmx.")) and isinstance(getattr(m, "lib", None), C.CDLL)]
    saved_lib = [(m, m.lib) for m in mods]
    saved_env = {k: os.environ.get(k) for k in env}
    try:
        for m in mods:
            m.lib = dl
        for k, v in env.items():
            os.environ[k] = str(v)
        yield dl
    finally:
        for m, lib in saved_lib:
            m.lib = lib
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
