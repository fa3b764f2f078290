"""SIFT extraction away from the reference setting: sfmx_sift_detect_compute (csrc/sift_features.hip)
bit-identical to oracle/sift_oracle.cpp -- keypoint rows byte for byte, descriptors array_equal -- with
nOctaveLayers, edgeThreshold and sigma set, so that every launch-time branch of detect_compute_impl runs:

  blur()            picks by the tap count n = cvRound(8 s + 1) | 1 of each layer's Gaussian:
                    blur_tile_n_kernel<n> for n in {11, 13, 17, 21, 27} (all the reference setting uses),
                    blur_tile_kernel for any other n <= 33, blur_row/col_kernel + dog_kernel above;
  small octaves     one fused launch (small_octaves_kernel) for the octaves of <= 2048 pixels when
                    nOctaveLayers + 3 <= 8 (SMALL_MAXL), per-octave launches otherwise;
  extrema scan      8 rows per thread when column blocks x rows x layers >= 65536, one row otherwise;
  descriptors       from the detection pyramid, or from a pyramid rebuilt un-doubled (all blur forms again);
  input             row pitch and base offset (up2_kernel, to_float_kernel), keypoint capacity.

The diagnostic library's switches turn the fused launch, the XCD block order and the rows-per-thread form
off and on; each variant must equal the oracle too, which is the bit identity their comments promise.
The tap counts each case relies on are asserted (`_taps`), so a case cannot drift off its branch unseen."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from oracle import oracle
import sift_cases

pytestmark = pytest.mark.gpu

SPECIALISED = {11, 13, 17, 21, 27}   # blur_tile_n_kernel<N> instantiations
RMAX = 16                            # blur_tile_kernel's largest radius
SMALL_MAXL = 8                       # small_octaves_kernel's tap slots
ECAPACITY = -4


@functools.lru_cache(maxsize=None)
def _image(name):
    if name == "blobs":      # keypoints on octaves -1 .. 3; its octaves of 37 x 47 pixels and below are "small"
        return sift_cases.blob_image(150, 190, n_blobs=100, seed=5)
    if name == "big":        # only large blobs: no keypoint of the doubled octave, descriptors from the rebuilt pyramid
        return sift_cases.big_blob_image(160, 200, seed=2)
    if name == "one":
        return sift_cases.single_blob_image(6.0)
    if name == "tall":
        return sift_cases.tall_blob_image(3700, 300)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _expected(name, **ok):
    """The oracle's (keypoints, descriptors) for a named image, computed once and shared (read only)."""
    k, d = oracle.sift(_image(name), **ok)
    k.setflags(write=False)
    d.setflags(write=False)
    return k, d


def _oracle_kw(kw):
    return {"nfeatures": kw.get("nfeatures", 0), "n_octave_layers": kw.get("nOctaveLayers", 3),
            "contrast_threshold": kw.get("contrastThreshold", 0.04), "edge_threshold": kw.get("edgeThreshold", 10.0),
            "sigma": kw.get("sigma", 1.6)}


def _check(name, **kw):
    """Host mode through the Python wrapper; contrast 0.04 unless given.  Every parameter reaches the oracle."""
    import sfmx
    kw = {"contrastThreshold": 0.04, **kw}
    k, d = sfmx.features.SIFT.create(**kw).detectAndCompute(_image(name))
    ek, ed = _expected(name, **_oracle_kw(kw))
    print(f"{name} {kw}: {len(ek)} keypoints, octaves {_octaves(ek)}, layers {_layers(ek)}")
    assert len(k) == len(ek), (len(k), len(ek))
    assert k.tobytes() == ek.tobytes()
    assert np.array_equal(d, ed)
    return ek


def _octaves(k):
    return sorted(set((k["octave"] & 255).astype(np.int8).tolist()))


def _layers(k):
    return sorted(set(((k["octave"] >> 8) & 255).tolist()))


def _taps(L, sigma):
    """Tap counts of kern[0 .. L + 3] of detect_compute_impl: the base blur, layers 1 .. L + 2, and the
    un-doubled base blur (getGaussianKernel's size rule, restated here only to name the branches)."""
    n = lambda s: int(round(8 * s + 1)) | 1   # noqa: E731  (round half to even, as cvRound)
    k = 2 ** (1 / L)
    out = [n(math.sqrt(max(sigma * sigma - 1.0, 0.01)))]
    for i in range(1, L + 3):
        prev = k ** (i - 1) * sigma
        out.append(n(math.sqrt((prev * k) ** 2 - prev ** 2)))
    return out + [n(math.sqrt(max(sigma * sigma - 0.25, 0.01)))]


def _forms(L, sigma):
    t = _taps(L, sigma)[:-1]
    return ({n for n in t if n in SPECIALISED}, {n for n in t if n not in SPECIALISED and n // 2 <= RMAX},
            {n for n in t if n // 2 > RMAX})


# B.1 ------------------------------------------------------------------ nOctaveLayers
# L: (taps on blur_tile_kernel, taps on the two-pass kernels, fused small-octave launch); sigma 1.6.
# The base blur (11 taps) and whatever is left run on blur_tile_n_kernel.
LAYER_CASES = {
    # 23 | 45, 91: radius 45 exceeds the small octaves' sides (37 x 47 and below), so reflect101 reflects
    # more than once, inside the fused launch
    1: ({23}, {45, 91}, True),
    2: ({15, 19}, {37}, True),        # 27 specialised
    4: ({9, 15}, set(), True),        # 11, 13, 17, 21 specialised
    5: ({9, 15, 19}, set(), True),    # L + 3 = SMALL_MAXL: the fused launch with all eight tap slots in use
    6: ({9, 15}, set(), False),       # L + 3 > SMALL_MAXL: every octave as per-octave launches
    8: ({7, 9}, set(), False),        # the same, 11 layers an octave
}


@pytest.mark.parametrize("L", sorted(LAYER_CASES))
def test_octave_layers(L):
    generic, two_pass, fused = LAYER_CASES[L]
    sp, ge, tp = _forms(L, 1.6)
    assert (ge, tp) == (generic, two_pass) and sp and (L + 3 <= SMALL_MAXL) == fused
    ek = _check("blobs", nOctaveLayers=L)
    assert 29 <= len(ek) <= 43
    assert _layers(ek) == list(range(1, L + 1))            # every inner layer yields a keypoint
    assert min(_octaves(ek)) == -1 and max(_octaves(ek)) >= 2   # doubled octave .. the fused launch's octaves


def test_sixteen_octave_layers():
    """The largest accepted layer count: 19 layers an octave of 5 .. 9 taps (blur_tile_kernel) and the
    specialised 11; per-octave launches."""
    sp, ge, tp = _forms(16, 1.6)
    assert (sp, ge, tp) == ({11}, {5, 7, 9}, set())
    ek = _check("one", nOctaveLayers=16)
    assert len(ek) > 0 and max(_layers(ek)) > 8


@pytest.mark.parametrize("kw", [{"nOctaveLayers": 0}, {"nOctaveLayers": 17}, {"edgeThreshold": 0.0}, {"sigma": 0.0}])
def test_rejected_parameters(kw):
    import sfmx
    with pytest.raises(ValueError):
        sfmx.features.SIFT.create(**kw).detectAndCompute(_image("one"))


# B.2 ------------------------------------------------------------------ edgeThreshold
@pytest.mark.parametrize("edge,count", [(1.2, 6), (2.0, 20), (3.0, 30), (50.0, 35)])
def test_edge_threshold(edge, count):
    assert len(_check("blobs", edgeThreshold=edge)) == count


# B.3 ------------------------------------------------------------------ sigma
# sigma, L: (blur_tile_kernel taps, two-pass taps, whether the oracle keeps a keypoint of the doubled octave)
SIGMA_CASES = {
    # 0.8: the base blur's sigma is the sig_diff clamp sqrt(0.01) -> 3 taps; no kept keypoint of the doubled
    # octave on this image, so the descriptors come from the rebuilt pyramid (7-tap base blur)
    (0.8, 3): ({3, 7, 9}, set(), False),
    (1.0, 3): ({3, 7, 9}, set(), True),
    (2.4, 3): ({19, 25, 31}, {39}, True),             # 17, 21 specialised
    (2.4, 6): ({15, 19, 23}, set(), True),            # per-octave launches; 11, 13, 17, 21 specialised
}


@pytest.mark.parametrize("sigma,L", sorted(SIGMA_CASES))
def test_sigma(sigma, L):
    generic, two_pass, doubled = SIGMA_CASES[(sigma, L)]
    _, ge, tp = _forms(L, sigma)
    assert (ge, tp) == (generic, two_pass)
    ek = _check("blobs", sigma=sigma, nOctaveLayers=L)
    assert 29 <= len(ek) <= 43 and (min(_octaves(ek)) == -1) == doubled


# B.4 ------------------------------------------------------------------ un-doubled descriptor pyramid
@pytest.mark.parametrize("L", [1, 6])
def test_undoubled_descriptor_pyramid(L):
    """compute() rebuilds the pyramid from firstOctave = 0 into the slots (o + 1) * (L + 3) + i of the
    detection pyramid; L = 1 takes it through the tile, specialised (13-tap base) and two-pass blurs."""
    ek = _check("big", nOctaveLayers=L)
    assert len(ek) > 0 and min(_octaves(ek)) >= 0


# B.5 ------------------------------------------------------------------ row pitch and base offset
def _abi(image_ptr, w, h, pitch, on_device, kp_ptr, desc_ptr, capacity, **kw):
    """sfmx_sift_detect_compute itself -> (return code, *n_keypoints)."""
    import sfmx
    s = sfmx.features.SIFT.create(**kw)
    n = C.c_int32(-1)
    rc = sfmx.features.lib.sfmx_sift_detect_compute(image_ptr, w, h, pitch, C.byref(s.params), on_device, 0, None, kp_ptr,
                                                    desc_ptr, capacity, C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("name", ["blobs", "big"])   # up2_kernel only | to_float_kernel as well
def test_pitch_and_offset_device(name):
    import torch
    import sfmx
    img = _image(name)
    h, w = img.shape
    big, _ = sift_cases.padded(img, left=3, right=5)
    dev = torch.device("cuda:0")
    view = torch.from_numpy(big).to(dev)[:, 3:3 + w]
    assert view.stride(0) == w + 8 and view.data_ptr() % 4 == 3
    kt = torch.zeros((256, 7), dtype=torch.int32, device=dev)
    dt = torch.zeros((256, 128), dtype=torch.float32, device=dev)
    n = sfmx.features.SIFT.create(contrastThreshold=0.04).detectAndCompute_device(view, kt, dt)
    torch.cuda.synchronize()
    ek, ed = _expected(name, **_oracle_kw({}))
    assert n == len(ek) > 0
    assert kt[:n].cpu().numpy().tobytes() == ek.tobytes()
    assert np.array_equal(dt[:n].cpu().numpy(), ed)


@pytest.mark.parametrize("name", ["blobs", "big"])
def test_pitch_and_offset_host(name):
    from sfmx.features import KEYPOINT_DTYPE
    img = _image(name)
    h, w = img.shape
    _, view = sift_cases.padded(img, left=3, right=5)
    assert view.strides[0] == w + 8 and not view.flags["C_CONTIGUOUS"]
    ek, ed = _expected(name, **_oracle_kw({}))
    k = np.zeros(256, KEYPOINT_DTYPE)
    d = np.zeros((256, 128), np.float32)
    rc, n = _abi(view.ctypes.data, w, h, view.strides[0], 0, k.ctypes.data, d.ctypes.data, 256, contrastThreshold=0.04)
    assert rc == 0 and n == len(ek) > 0
    assert k[:n].tobytes() == ek.tobytes() and np.array_equal(d[:n], ed)


# B.6 ------------------------------------------------------------------ 8 rows per thread
def test_extrema_rows_per_thread_full_set():
    """3700 x 300: octave 0 of the doubled pyramid has 3 column blocks x 7390 rows x 3 layers = 66510 >=
    65536 scan items, so each thread takes 8 rows, and 7390 % 8 = 6 leaves a partial last row group.  With
    nfeatures = 0 every keypoint is compared: a missed or doubled extremum anywhere shows."""
    h, w = _image("tall").shape
    nbx, hr = (2 * w - 10 + 255) // 256, 2 * h - 10
    assert nbx * hr * 3 >= 65536 and hr % 8 == 6
    ek = _check("tall")
    doubled = ek[(ek["octave"] & 255) == 255]              # the octave the 8-row form scans
    assert len(ek) > 3000 and len(doubled) > 800
    # the last row group is rows 7389 .. 7394 of the doubled image: y >= 3694.5 here
    assert np.count_nonzero(doubled["y"] >= (5 + hr // 8 * 8) / 2) >= 3


# B.7 ------------------------------------------------------------------ capacity
def test_capacity_host():
    from sfmx.features import KEYPOINT_DTYPE
    img = _image("blobs")
    ek, ed = _expected("blobs", **_oracle_kw({}))
    cap = len(ek) // 2
    k = np.frombuffer(bytes([0x5A]) * (KEYPOINT_DTYPE.itemsize * (cap + 4)), KEYPOINT_DTYPE).copy()
    d = np.full((cap + 4, 128), -7.0, np.float32)
    rc, n = _abi(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], 0, k.ctypes.data, d.ctypes.data, cap,
                 contrastThreshold=0.04)
    assert rc == ECAPACITY and n == len(ek)
    assert k[:cap].tobytes() == ek[:cap].tobytes() and np.array_equal(d[:cap], ed[:cap])
    assert k[cap:].tobytes() == bytes([0x5A]) * (KEYPOINT_DTYPE.itemsize * 4) and np.all(d[cap:] == -7.0)


def test_capacity_device():
    import torch
    img = _image("blobs")
    ek, ed = _expected("blobs", **_oracle_kw({}))
    cap = len(ek) // 2
    dev = torch.device("cuda:0")
    ti = torch.from_numpy(img).to(dev)
    kt = torch.full((cap + 4, 7), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    dt = torch.full((cap + 4, 128), -7.0, dtype=torch.float32, device=dev)
    rc, n = _abi(ti.data_ptr(), img.shape[1], img.shape[0], ti.stride(0), 1, kt.data_ptr(), dt.data_ptr(), cap,
                 contrastThreshold=0.04)
    torch.cuda.synchronize()
    assert rc == ECAPACITY and n == len(ek)
    assert kt[:cap].cpu().numpy().tobytes() == ek[:cap].tobytes()
    assert np.array_equal(dt[:cap].cpu().numpy(), ed[:cap])
    assert bool((kt[cap:] == 0x5A5A5A5A).all()) and bool((dt[cap:] == -7.0).all())


# C -------------------------------------------------------------------- diagnostic library: the bit-identity claims
@pytest.mark.parametrize("env,kw", [
    ({"SFMX_SIFT_SMALL": 0}, {}),                          # the small octaves as per-octave launches, L = 3
    ({"SFMX_SIFT_SMALL": 0}, {"nOctaveLayers": 5}),        # and at the layer count that fills the tap slots
    ({"SFMX_SIFT_SMALL_PX": 32768}, {}),                   # octave 1 (150 x 190) inside the fused launch
    ({"SFMX_SIFT_SMALL_PX": 1}, {}),                       # nothing fused
    ({"SFMX_SIFT_XCD": 0}, {}),                            # the tile blurs on the plain grid
    ({"SFMX_SIFT_XCD_EXTREMA": 1}, {}),                    # the extrema scan on the XCD block order
], ids=lambda v: "-".join(f"{a}={b}" for a, b in v.items()) or "default")
def test_launch_variants_equal_the_oracle(env, kw):
    from diag import diagnostic
    with diagnostic(**env):
        ek = _check("blobs", **kw)
    assert len(ek) >= 35 and max(_octaves(ek)) == 3


@pytest.mark.parametrize("rows", [1, 3])   # one row per thread | 7390 % 3 = 1: another partial last group
def test_extrema_rows_variants_equal_the_oracle(rows):
    from diag import diagnostic
    with diagnostic(SFMX_SIFT_EX_ROWS=rows):
        ek = _check("tall")
    assert len(ek) > 3000
