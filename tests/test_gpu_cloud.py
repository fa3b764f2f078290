"""GPU parity for the point-cloud neighbour search (PclUtils::getNearestNeighbors and the loops around it,
PclUtils.cpp:75-136): the grid search of csrc/cloud.hip through sfmx.cloud against the brute-force float32
restatement tests/cloud_ref.py.  out_distance is compared as uint64 bit patterns (one correctly rounded fp64
square root of the same float on both sides), out_neighbor exactly."""
import numpy as np
import pytest
import torch

from sfmx import cloud
import cloud_ref

pytestmark = pytest.mark.gpu

_CACHE = {}


def expected(name, xyz, max_equal=0):
    """The restatement, computed once per (case, max_equal) and left unchanged."""
    if (name, max_equal) not in _CACHE:
        d, nb = cloud_ref.neighbor_distances(xyz, max_equal)
        d.setflags(write=False)
        nb.setflags(write=False)
        _CACHE[name, max_equal] = (d, nb)
    return _CACHE[name, max_equal]


def check(xyz, exp, max_equal=0):
    d, nb = cloud.neighbor_distances(xyz, max_equal, neighbors=True)
    ed, enb = exp
    assert d.dtype == np.float64 and nb.dtype == np.int64 and d.shape == ed.shape and nb.shape == enb.shape
    bad = np.flatnonzero(d.view(np.uint64) != ed.view(np.uint64))
    assert len(bad) == 0, (len(bad), bad[:8], d[bad[:8]], ed[bad[:8]])
    bad = np.flatnonzero(nb != enb)
    assert len(bad) == 0, (len(bad), bad[:8], nb[bad[:8]], enb[bad[:8]])
    only = cloud.neighbor_distances(xyz, max_equal)          # out_neighbor = NULL
    assert np.array_equal(only.view(np.uint64), ed.view(np.uint64))
    return cloud.last_stats()


def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


@pytest.mark.parametrize("max_equal", [0, 2])
def test_uniform_cube(max_equal):
    x = uniform(4096, 3)
    st = check(x, expected("cube", x, max_equal), max_equal)
    assert st["kernel_ms"] > 0 and st["evaluations"] >= 4096


def test_outliers_do_not_flatten_the_grid():
    """Four far points on different axes: a grid on the raw bounding box holds the cluster in one cell and
    evaluates about n^2 distances.  The bound is a condition on the design, not a measurement."""
    x = uniform(8192, 5)
    far = np.zeros((4, 3), np.float32)
    far[0, 0], far[1, 1], far[2, 2], far[3, 0] = 1e3, 1e4, 1e5, 1e6
    x = np.concatenate([x, far])
    n = len(x)
    assert n == 8196
    st = check(x, expected("outliers", x))
    print("evaluations", st["evaluations"], "brute", st["brute_queries"], "n^2/8", n * n // 8)
    assert st["evaluations"] <= n * n // 8
    assert st["brute_queries"] >= 4          # the far points cannot be certified by two rings of cells


def duplicated_points():
    rng = np.random.default_rng(11)
    base = np.unique(rng.integers(-20, 20, size=(400, 3)), axis=0)
    base = base[rng.permutation(len(base))[:300]]
    copies = rng.integers(1, 4, size=len(base))
    x = np.repeat(base, copies, axis=0).astype(np.float32)
    perm = rng.permutation(len(x))
    return x[perm], np.repeat(copies, copies)[perm]


@pytest.mark.parametrize("max_equal", [0, 1, 2])
def test_duplicates(max_equal):
    x, copies = duplicated_points()
    assert len(np.unique(x, axis=0)) == 300
    exp = expected("dup", x, max_equal)
    check(x, exp, max_equal)
    ke = min(2 + max_equal, len(x))
    d = cloud.neighbor_distances(x, max_equal)
    assert np.array_equal(d == 0, copies >= ke)       # zeros exactly where z >= Ke


def test_identical_points_and_tiny_clouds():
    x = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (1000, 1))
    d, nb = cloud.neighbor_distances(x, 0, neighbors=True)
    assert not d.any() and (nb == -1).all()
    d, nb = cloud.neighbor_distances(np.zeros((0, 3), np.float32), neighbors=True)
    assert d.shape == (0,) and nb.shape == (0,)
    d, nb = cloud.neighbor_distances(np.array([[1, 2, 3]], np.float32), neighbors=True)
    assert d.tolist() == [0.0] and nb.tolist() == [-1]
    assert cloud.last_stats()["kernel_ms"] == 0           # n <= 1 launches nothing
    two = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    d, nb = cloud.neighbor_distances(two, neighbors=True)
    assert d.tolist() == [5.0, 5.0] and nb.tolist() == [1, 0]
    d, nb = cloud.neighbor_distances(two[[0, 0]], neighbors=True)
    assert d.tolist() == [0.0, 0.0] and nb.tolist() == [-1, -1]


def test_subnormals_are_kept():
    x = np.array([(0, 0, 0), (1e-23, 0, 0), (5, 0, 0), (5, 1e-20, 0), (9, 9, 9)], np.float32)
    exp = expected("subnormal", x)
    assert exp[1].tolist() == [-1, -1, 3, 2, 2]
    assert exp[0][0] == 0 and exp[0][1] == 0 and abs(exp[0][2] - 1e-20) < 1e-25 and abs(exp[0][4] - 13.34) < 0.01
    check(x, exp)


def test_points_on_a_line():
    t = np.random.default_rng(7).random(512).astype(np.float32)
    x = np.stack([np.full(512, 2.5, np.float32), t * 40 - 3, np.full(512, -1.0, np.float32)], 1)
    check(x, expected("line", x))


def test_points_on_a_plane():
    x = uniform(3000, 9)
    x[:, 2] = 0.125
    check(x, expected("plane", x))


@pytest.mark.parametrize("seed", [None, 2])
def test_lattice_ties(seed):
    """Every point of an integer lattice has up to six neighbours at the same distance: the smallest index
    wins, inside one cell or across cells.  The expected values are analytic (cloud_ref.lattice_case)."""
    x, d, nb = cloud_ref.lattice_case(16, 1.0, (-3.0, 0.0, 5.0), seed)
    check(x, (d, nb))
    x, d, nb = cloud_ref.lattice_case(9, 0.5, (100.0, -7.0, 0.25), seed)
    check(x, (d, nb))


def test_non_finite_points_are_left_out():
    x = uniform(700, 13)
    x[5, 0] = np.nan
    x[77, 2] = np.inf
    x[300] = (-np.inf, np.nan, 0)
    exp = expected("nonfinite", x)
    assert exp[0][[5, 77, 300]].tolist() == [0, 0, 0] and exp[1][[5, 77, 300]].tolist() == [-1, -1, -1]
    assert not np.isin(exp[1], [5, 77, 300]).any()
    check(x, exp)
    allnan = np.full((70, 3), np.nan, np.float32)
    d, nb = cloud.neighbor_distances(allnan, neighbors=True)
    assert not d.any() and (nb == -1).all()


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 1025])
def test_sizes_around_wave_and_block_edges(n):
    x = uniform(n, 100 + n)
    check(x, expected("n%d" % n, x))


@pytest.mark.parametrize("scale", [1e-30, 3e19])
def test_extreme_scales(scale):
    """1e-30: the stop bound underflows, every query is resolved by coverage or brute force.  3e19: far pairs
    overflow d to +inf (a positive d), near pairs do not."""
    x = (uniform(600, 21).astype(np.float64) * scale).astype(np.float32)
    check(x, expected("scale%g" % scale, x))


def test_surface_cloud_many_points_per_cell():
    """Points on a noisy sphere and a plane: tens of points per occupied cell, several blocks."""
    rng = np.random.default_rng(17)
    v = rng.normal(size=(8000, 3))
    sphere = v / np.linalg.norm(v, axis=1, keepdims=True) * (1 + 0.002 * rng.normal(size=(8000, 1)))
    plane = np.concatenate([rng.random((4000, 2)) * 3 - 1.5, 0.001 * rng.normal(size=(4000, 1)) - 1.2], 1)
    x = np.concatenate([sphere, plane]).astype(np.float32)
    x = x[rng.permutation(len(x))]
    st = check(x, expected("surface", x))
    print("surface: evaluations per point", st["evaluations"] / len(x), "brute", st["brute_queries"])


def test_scattered_points_go_through_the_brute_force_kernel():
    """A dense cluster and 51 points scattered 100 times as wide: the box follows the cluster, the scattered
    points sit in border cells that two rings cannot certify.  Several groups of queries, the last one partial."""
    rng = np.random.default_rng(23)
    x = np.concatenate([rng.random((2000, 3)), rng.random((51, 3)) * 100 - 50]).astype(np.float32)
    x = x[rng.permutation(len(x))]
    st = check(x, expected("scattered", x))
    print("scattered: brute", st["brute_queries"], "evaluations", st["evaluations"])
    assert st["brute_queries"] >= 5


def test_device_tensor_input():
    x = uniform(4096, 3)
    ed, enb = expected("cube", x, 0)
    t = torch.from_numpy(x).cuda()
    d, nb = cloud.neighbor_distances(t, 0, neighbors=True)
    assert d.is_cuda and nb.is_cuda
    assert np.array_equal(d.cpu().numpy().view(np.uint64), ed.view(np.uint64)) and np.array_equal(nb.cpu().numpy(), enb)
    d = cloud.neighbor_distances(t[:1])
    assert d.cpu().tolist() == [0.0]


def test_argument_errors():
    from sfmx import _lib
    assert _lib.lib.sfmx_cloud_neighbor_distances(None, -1, 0, 0, 0, None, None, None) == _lib.SFMX_EINVAL
    assert _lib.lib.sfmx_cloud_neighbor_distances(None, 5, 0, 0, 0, None, None, None) == _lib.SFMX_EINVAL
    x = uniform(8, 1)
    with pytest.raises(ValueError):
        cloud.neighbor_distances(x, device=63)
    d0 = cloud.neighbor_distances(x, -5)                    # max(0, maxEqual)
    assert np.array_equal(d0, cloud.neighbor_distances(x, 0))
