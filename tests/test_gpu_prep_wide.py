"""GPU: every array the batched SIFT prepare kernel writes (prep_l2_batch_kernel), read back through the diagnostic
library (sfmx_diag_matcher_prep_rows, sfmx_diag_matcher_prep_rows8) and compared value for value with the int8
definitions (desc8 = u - 128, norm = |u - 128|^2, the two integer keys) and with the numpy restatement of the FP6
quantiser and row packing (tests/sift_fp6_ref.py: desc6, keyf, (|a|^2, |e|^2), the image maxima); pad rows are zero
rows with the pad keys.

Whatever form the kernel takes, these arrays do not change.  The cases were chosen for a row function with 8 lanes
per row and 16 columns per lane for full 128-column rows of a 16-byte aligned source (measured slower than the
32-lane one and not kept), and hold for any form that treats such rows apart: row counts 1, 7, 8, 9,
63, 64, 65 sit around the 8 rows of a wave and the 64 rows of a workgroup; a 100-column image and a device source
at a 4-byte but not 16-byte aligned address are the inputs such a form must leave to the general row function;
two images of one call have different maxima; an image with one non-integral value sets its flag, and its pair
equals the oracle's fp32 result.
Fails without the feature: the diagnostic library has no reader of the int8 rows."""
import ctypes as C

import numpy as np
import pytest

import sfmx
import sift_fp6_ref as ref
from sfmx import synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

PAD_KEYF = np.float32(-1.0e30)
PAD_KEY2 = np.int32(-0x3F3F3F40)          # 0xC0C0C0C0
INT_MIN = np.int32(-2**31)
ROW_COUNTS = (1, 7, 8, 9, 63, 64, 65)


def _read(dl, m, i):
    f6, f8 = dl.sfmx_diag_matcher_prep_rows, dl.sfmx_diag_matcher_prep_rows8
    f6.restype, f6.argtypes = C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    f8.restype, f8.argtypes = C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    n_pad = f6(m._h, i, None, None, None, None, None)
    assert n_pad > 0 and n_pad % 64 == 0
    a = {"desc6": np.zeros((n_pad, 24), np.uint32), "keyf": np.zeros(n_pad, np.float32), "ne": np.zeros((n_pad, 2), np.int32),
         "norm": np.zeros(n_pad, np.int32), "imax": np.zeros(2, np.int32), "desc8": np.zeros((n_pad, 128), np.int8),
         "keyc": np.zeros(n_pad, np.int32), "keyc2": np.zeros(n_pad, np.int32)}
    assert f6(m._h, i, *(a[k].ctypes.data for k in ("desc6", "keyf", "ne", "norm", "imax"))) == n_pad
    assert f8(m._h, i, *(a[k].ctypes.data for k in ("desc8", "keyc", "keyc2"))) == n_pad
    return a


def _check(a, img, tag):
    n = len(img)
    assert len(a["norm"]) >= n
    u = np.full((n, 128), 128, np.int64)           # a missing column is the int8 form's zero, u = 128
    ok = (img >= 0) & (img <= 255) & (img == np.floor(img))
    u[:, :img.shape[1]] = np.where(ok, img, 128)   # so is a value that is no integer in 0..255
    v = u - 128
    n2 = (v * v).sum(1)
    r = np.arange(n)
    assert np.array_equal(a["desc8"][:n], v.astype(np.int8)), tag
    assert np.array_equal(a["norm"][:n], n2), tag
    assert np.array_equal(a["keyc"][:n], -(n2 << 8) + 255 - (r & 255)), tag
    assert np.array_equal(a["keyc2"][:n], -((n2 + 1) >> 1)), tag
    mq, e = ref.quantise(u)
    av = u - ref.OFFSET
    a2, e2 = (av * av).sum(1), (e * e).sum(1)
    assert np.array_equal(a["desc6"][:n], ref.pack_rows(mq)), tag
    assert np.array_equal(a["ne"][:n, 0], a2) and np.array_equal(a["ne"][:n, 1], e2), tag
    assert np.array_equal(a["keyf"][:n], (-a2.astype(np.float32) / np.float32(2048.0)).astype(np.float32)), tag
    assert np.array_equal(a["imax"], [e2.max(), a2.max()]), tag
    # pad rows
    assert (a["desc8"][n:] == 0).all() and (a["norm"][n:] == 0).all() and (a["desc6"][n:] == 0).all(), tag
    assert (a["keyc"][n:] == INT_MIN).all() and (a["keyc2"][n:] == PAD_KEY2).all(), tag
    assert (a["keyf"][n:] == PAD_KEYF).all() and (a["ne"][n:] == 0).all(), tag


def _images():
    rng = np.random.default_rng(6101)
    pool = synth.sift_images(1, 300, seed=6102, shared=0.0)[0]
    imgs = [pool[7 * k:7 * k + n].copy() for k, n in enumerate(ROW_COUNTS)]
    every = np.tile(np.arange(256, dtype=np.float32), 32).reshape(64, 128)                   # every value 0..255
    imgs.append(np.concatenate([ref.extreme_rows(), ref.midpoint_rows(), every]).astype(np.float32))   # bright: large maxima
    imgs.append(rng.integers(20, 45, (33, 128)).astype(np.float32))                          # dim: small maxima
    imgs.append(synth.sift_images(1, 40, seed=6103, shared=0.0)[0][:, :100].copy())          # narrow rows: 100 columns
    return imgs


def test_every_array_of_host_images():
    imgs = _images()
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            got = [_read(dl, m, i) for i in range(len(imgs))]
        finally:
            m.close()
    for i, (a, img) in enumerate(zip(got, imgs)):
        _check(a, img, i)
    bright, dim = got[len(ROW_COUNTS)]["imax"], got[len(ROW_COUNTS) + 1]["imax"]
    assert (bright > dim).all()                    # two images of one call with different maxima


def test_device_sources_aligned_and_not():
    torch = pytest.importorskip("torch")
    img = synth.sift_images(1, 73, seed=6111, shared=0.0)[0]
    big = torch.zeros(73 * 128 + 4, dtype=torch.float32, device="cuda")
    off = (16 - big.data_ptr() % 16) // 4 % 4 + 1            # first element 4 bytes past a 16-byte boundary
    shifted = big[off:off + 73 * 128].view(73, 128)
    shifted.copy_(torch.from_numpy(img))
    aligned = torch.from_numpy(img).cuda()
    assert shifted.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0 and shifted.is_contiguous()
    s = torch.cuda.current_stream().cuda_stream
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images_device([shifted, aligned], stream=s)
            torch.cuda.synchronize()
            got = [_read(dl, m, i) for i in range(2)]
        finally:
            m.close()
    for i, a in enumerate(got):
        _check(a, img, i)


def test_one_non_integral_value_sets_the_flag():
    from oracle import oracle
    rng = np.random.default_rng(6121)
    base = synth.sift_images(2, 200, seed=6122, shared=0.0)
    T = base[0].copy()
    Q = np.clip(T[rng.permutation(200)[:150]] + rng.integers(-5, 6, (150, 128)), 0, 255).astype(np.float32)
    Q[77, 50] += np.float32(0.5)                              # the one value
    imgs = [Q, T, base[1]]
    pairs = np.array([[0, 1], [1, 0], [2, 1]], np.int32)
    em, eoff = oracle.match_pairs(imgs, pairs, 0.7)
    assert eoff[1] > 100
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            m.run(pairs, 0.7, False, 0)
            got, off, _ = m.fetch()
            slow, f32 = m.stats()
            arrays = [_read(dl, m, i) for i in range(3)]
        finally:
            m.close()
    assert f32 == 2                                           # the flag: both pairs of image 0 took the fp32 path
    assert np.array_equal(off, eoff) and got.tobytes() == em.tobytes()
    for i, (a, img) in enumerate(zip(arrays, imgs)):
        _check(a, img, i)
