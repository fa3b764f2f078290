"""GPU: the batched SIFT prepare kernel finishes its own job.  Its workgroups leave their maxima in per-workgroup
slots, the last workgroup of an image reduces them into the image's imax words, and the last of those publishes the
integrality flags to the host and puts the flags and every ticket back to zero, so set_images issues no fill in
front of the kernel and no publishing kernel behind it.

What can go wrong is state that survives a call (a ticket, a flag, a slot or a maximum of the last set), a
workgroup counted for an image it has no rows of (the grid's x extent follows the largest image), and a host that
waits for a sequence word nobody stores.  So: every prepared array and imax of every image against the numpy
restatement (tests/test_gpu_prep_wide.py's reader and checker), for sets of 1, 2, 3 and 65 images (past the 64-word
alignment of the flag words) with 1, 63, 64, 65, 129 and 513 rows mixed in one set; one matcher re-used over sets
with large and small values, 65 and 2 images, one non-integral value and none, each call checked; and host sources,
whose set_images spins on the published word.
Fails without the feature only where the parent would: these arrays and results do not change with the kernel's form."""
import numpy as np
import pytest

import sfmx
from sfmx import synth
from diag import diagnostic
from test_gpu_prep_wide import _check, _read

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 129, 513)


@pytest.fixture(scope="module")
def pool():
    return synth.sift_images(1, 1400, seed=7301, shared=0.0)[0]


def _set(pool, n, first=0):
    """n images cut from the pool, row counts cycling through ROWS from `first` (every count in a set of 6 or more)."""
    return [pool[11 * k:11 * k + ROWS[(first + k) % len(ROWS)]].copy() for k in range(n)]


def _oracle(imgs, pairs, ratio=0.7):
    from oracle import oracle
    return oracle.match_pairs(imgs, pairs, ratio)


def _check_all(dl, m, imgs, tag):
    for i, img in enumerate(imgs):
        _check(_read(dl, m, i), img, (tag, i))


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_value_for_value_host_sets(pool, n):
    imgs = _set(pool, n, first=n)          # n = 1: 63 rows; 2: 64, 65; 3: 65, 129, 513: the grid exceeds most images' rows
    if n == 3:
        imgs.append(pool[900:940, :100].copy())   # narrow rows: 100 columns
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images(imgs)
            _check_all(dl, m, imgs, n)
        finally:
            m.close()


def _to_device(torch, imgs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in imgs]


def test_value_for_value_device_sources(pool):
    torch = pytest.importorskip("torch")
    imgs = _set(pool, 7, first=5)          # 513, 1, 63, 64, 65, 129, 513 rows
    imgs.append(pool[900:940, :100].copy())
    dev = _to_device(torch, imgs)
    big = torch.zeros(129 * 128 + 4, dtype=torch.float32, device="cuda")
    off = (16 - big.data_ptr() % 16) // 4 % 4 + 1          # first element 4 bytes past a 16-byte boundary
    shifted = big[off:off + 129 * 128].view(129, 128)
    shifted.copy_(torch.from_numpy(pool[300:429]))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    imgs.append(pool[300:429])
    dev.append(shifted)
    s = torch.cuda.current_stream().cuda_stream
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            m.set_images_device(dev, stream=s)
            torch.cuda.synchronize()
            _check_all(dl, m, imgs, "device")
        finally:
            m.close()


def test_one_matcher_reused(pool):
    """Each call checked: nothing of the last set (a maximum, a slot, a ticket, a flag) shows in the next."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(7311)
    shapes = (65, 129, 513)
    large = [rng.integers(150, 256, (r, 128)).astype(np.float32) for r in shapes]
    small = [rng.integers(30, 40, (r, 128)).astype(np.float32) for r in shapes]
    many = _set(pool, 65)
    two = _set(pool, 2, first=4)                       # 129 and 513 rows
    match = synth.sift_images(3, 150, seed=7312, shared=0.5)
    frac = [a.copy() for a in match]
    frac[1][77, 50] += np.float32(0.5)                  # exactly one non-integral value, in image 1
    pairs = sfmx.pairs_unordered(3)
    exp_frac, exp_int = _oracle(frac, pairs), _oracle(match, pairs)
    assert exp_int[1][-1] > 30
    s = torch.cuda.current_stream().cuda_stream
    with diagnostic() as dl:
        m = sfmx.BFMatcher(sfmx.NORM_L2)
        try:
            imax = []
            for tag, imgs in (("large", large), ("small", small), ("65", many), ("2", two)):
                dev = _to_device(torch, imgs)
                m.set_images_device(dev, stream=s)
                torch.cuda.synchronize()
                _check_all(dl, m, imgs, tag)            # imax among them: read directly, stale maxima leave the matches equal
                imax.append(np.array([_read(dl, m, i)["imax"] for i in range(len(imgs))]))
            assert (imax[1] < imax[0]).all()            # the maxima fell with the values
            for imgs, (em, eoff), n_f32 in ((frac, exp_frac, 2), (match, exp_int, 0)):
                dev = _to_device(torch, imgs)
                m.set_images_device(dev, stream=s)
                m.run(pairs, 0.7, False, 0, stream=s)
                got, off, _ = m.fetch(stream=s)
                assert m.stats(stream=s)[1] == n_f32    # only image 1's flag: its two pairs on the fp32 fallback, then none
                assert np.array_equal(off, eoff) and got.tobytes() == em.tobytes()
                _check_all(dl, m, imgs, ("run", n_f32))
        finally:
            m.close()


@pytest.mark.parametrize("fractional", [False, True])
def test_host_sources_return_and_match_the_oracle(fractional):
    """set_images spins on the word the kernel's last workgroup publishes: it must return, with the right flags."""
    imgs = [a.copy() for a in synth.sift_images(3, 150, seed=7321, shared=0.5)]
    imgs[2] = imgs[2][:65]
    if fractional:
        imgs[0][3, 9] += np.float32(0.25)
    pairs = sfmx.pairs_unordered(3)
    em, eoff = _oracle(imgs, pairs)
    m = sfmx.BFMatcher(sfmx.NORM_L2)
    try:
        for _ in range(2):                              # twice: the second call starts from what the first left
            m.set_images(imgs)
            m.run(pairs, 0.7, False, 0)
            got, off, _ = m.fetch()
            assert m.stats()[1] == (2 if fractional else 0)
            assert np.array_equal(off, eoff) and got.tobytes() == em.tobytes()
    finally:
        m.close()
