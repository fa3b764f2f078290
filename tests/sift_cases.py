"""Synthetic grayscale images for the SIFT extraction row:
Gaussian blobs of several scales and contrasts on a smooth background, plus
mild noise, so the detector finds extrema on several octaves."""
import numpy as np


def blob_image(h, w, n_blobs=40, seed=0, noise=2.0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 100 + 30 * np.sin(xx / 37.0) * np.cos(yy / 29.0)
    for _ in range(n_blobs):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        s = rng.uniform(1.5, min(h, w) / 10)
        a = rng.uniform(-90, 90)
        sx, sy = s, s * rng.uniform(0.5, 1.0)
        img += a * np.exp(-(((xx - cx) / sx) ** 2 + ((yy - cy) / sy) ** 2) / 2)
    img += rng.normal(0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def big_blob_image(h, w, seed=0, n=12, smin=8.0, smax=20.0):
    """Only large blobs on a flat background: every keypoint comes from octave >= 0, so
    SIFT::compute (called after detect, SfM.cpp:586-587) rebuilds an un-doubled pyramid
    (firstOctave = 0) for the descriptors."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 110.0)
    for _ in range(n):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        s = rng.uniform(smin, smax)
        img += rng.uniform(-90, 90) * np.exp(-(((xx - cx) / s) ** 2 + ((yy - cy) / s) ** 2) / 2)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def single_blob_image(s=6.0, h=96, w=128, cx=70.3, cy=41.6):
    """One isotropic Gaussian blob of standard deviation `s`, amplitude 150 on a flat 60."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(np.rint(60 + 150 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s ** 2))), 0, 255).astype(np.uint8)


def tall_blob_image(h=3700, w=300, tile_h=40, n_blobs=40, seed=31, start=28):
    """h x w from one tile_h x w blob_image stacked alternately upright and flipped (so the seams are
    continuous), rows start .. start + h: tall enough for the extrema scan's rows-per-thread form
    (3 column blocks x 7390 rows x 3 layers >= 65536) at a fraction of blob_image's cost.  The low tile
    keeps the blobs small (sigma 1.5 .. 4), so a quarter of the ~3200 keypoints come from the doubled octave,
    the only one that scan form runs on; with the default start five of them lie in the last 3 rows above
    the border."""
    tile = blob_image(tile_h, w, n_blobs=n_blobs, seed=seed)
    reps = -(-(start + h) // tile_h)
    stack = np.concatenate([tile if i % 2 == 0 else tile[::-1] for i in range(reps)])
    return np.ascontiguousarray(stack[start:start + h])


def padded(img, left=3, right=5, seed=99):
    """-> (big, view): `view` equals `img` and lies inside the wider random-filled `big`, `left` bytes
    into each row, so view's row pitch is img's width + left + right and its base is offset."""
    h, w = img.shape
    big = np.random.default_rng(seed).integers(0, 256, (h, w + left + right), dtype=np.uint8)
    big[:, left:left + w] = img
    return big, big[:, left:left + w]


def big_photo_37mp():
    """6144 x 6144 u8: noisy flat background plus six 512 x 512 blob patches (fixture
    tests/golden/sift_37mp.npz, generator tests/golden/make_sift_big.py)."""
    rng = np.random.default_rng(37)
    img = np.clip(np.rint(rng.normal(120, 2.0, (6144, 6144))), 0, 255).astype(np.uint8)
    for i, (y, x) in enumerate([(300, 400), (300, 5000), (2900, 2800), (5400, 700), (5300, 5300), (4000, 3900)]):
        img[y:y + 512, x:x + 512] = blob_image(512, 512, n_blobs=120, seed=100 + i)
    return img
