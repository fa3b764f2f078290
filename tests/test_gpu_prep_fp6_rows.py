"""GPU: what the batched SIFT prepare kernel (prep_l2_batch_kernel) writes, read back through the diagnostic
library (sfmx_diag_matcher_prep_rows) and compared value for value with the numpy restatement of the FP6
quantiser and row packing (tests/sift_fp6_ref.py): packed e2m3 rows, the C operand keyf, (|a|^2, |e|^2), the
int8 norm and the image maxima; pad rows are zero rows with the pad key.  Whatever form the kernel takes, these
arrays do not change.
Fails without the feature: the diagnostic library has no such reader."""
import ctypes as C

import numpy as np
import pytest

import sfmx
import sift_fp6_ref as ref
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

PAD_KEY = np.float32(-1.0e30)


def _images():
    rng = np.random.default_rng(4101)
    every = np.tile(np.arange(256, dtype=np.float32), 64)[:128 * 100].reshape(100, 128)     # every value 0..255
    return [synth.sift_images(1, 301, seed=4102, shared=0.0)[0],                              # an odd row count
            np.concatenate([ref.extreme_rows(), ref.midpoint_rows(), every]).astype(np.float32),
            rng.integers(0, 256, (65, 128)).astype(np.float32),                               # one row past a workgroup
            synth.sift_images(1, 40, seed=4103, shared=0.0)[0][:, :100].copy()]               # narrow rows: 100 columns


def test_prepared_rows_equal_the_restatement():
    imgs = _images()
    with diagnostic() as dl:
        fn = dl.sfmx_diag_matcher_prep_rows
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            for i, img in enumerate(imgs):
                n_pad = fn(m._h, i, None, None, None, None, None)
                assert n_pad >= len(img) and n_pad % 64 == 0
                desc6 = np.zeros((n_pad, 24), np.uint32)
                keyf = np.zeros(n_pad, np.float32)
                ne = np.zeros((n_pad, 2), np.int32)
                norm = np.zeros(n_pad, np.int32)
                imax = np.zeros(2, np.int32)
                assert fn(m._h, i, *(a.ctypes.data for a in (desc6, keyf, ne, norm, imax))) == n_pad
                n = len(img)
                u = np.full((n, 128), 128, np.int64)           # a missing column is the int8 form's zero, u = 128
                u[:, :img.shape[1]] = img
                mq, e = ref.quantise(u)
                a = u - ref.OFFSET
                a2, e2 = (a * a).sum(1), (e * e).sum(1)
                assert np.array_equal(desc6[:n], ref.pack_rows(mq)), i
                assert np.array_equal(ne[:n, 0], a2) and np.array_equal(ne[:n, 1], e2), i
                assert np.array_equal(keyf[:n], (-a2.astype(np.float32) / np.float32(2048.0)).astype(np.float32)), i
                assert np.array_equal(norm[:n], ((u - 128) ** 2).sum(1)), i
                assert (desc6[n:] == 0).all() and (keyf[n:] == PAD_KEY).all() and (ne[n:] == 0).all() and (norm[n:] == 0).all()
                assert np.array_equal(imax, [e2.max(), a2.max()]), i
        finally:
            m.close()
