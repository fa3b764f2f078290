"""CPU: the numpy restatement of the neighbour search (tests/cloud_ref.py) against an independent anchor, a
float64 k-d tree, and against the reference's literal "sort, take K, first positive" form."""
import numpy as np
import pytest

import cloud_ref


def test_restatement_agrees_with_a_float64_kd_tree():
    """d is four float roundings away from the exact squared distance (three of them on the sum, one on the
    largest square), a relative 4 * 2^-24; the square root halves it: 2^-23 on the distance, 2^-21 with a factor 2
    of slack and the tree's own float64 rounding."""
    spatial = pytest.importorskip("scipy.spatial")
    x = np.random.default_rng(3).random((4096, 3)).astype(np.float32)
    d, nb = cloud_ref.neighbor_distances(x)
    td, ti = spatial.cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k=2)
    rel = np.abs(d - td[:, 1]) / td[:, 1]
    print("max relative difference", rel.max())
    assert rel.max() <= 2.0 ** -21
    assert (nb == ti[:, 1]).mean() > 0.999          # the nearest point itself, up to float ties


def test_offset_cloud_differences_are_exact():
    """The same kind of cloud moved by +1000 per axis: coordinates are multiples of 2^-14, so every dx is exact;
    the agreement with float64 stays within the same bound, and the distances are those of the float coordinates."""
    spatial = pytest.importorskip("scipy.spatial")
    x = (np.random.default_rng(4).random((4096, 3)) + 1000.0).astype(np.float32)
    d, _ = cloud_ref.neighbor_distances(x)
    td, _ = spatial.cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k=2)
    assert (np.abs(d - td[:, 1]) <= td[:, 1] * 2.0 ** -21).all()


@pytest.mark.parametrize("max_equal", [0, 1, 2, 5])
def test_reduction_equals_the_literal_form(max_equal):
    rng = np.random.default_rng(12)
    base = np.unique(rng.integers(-4, 5, size=(90, 3)), axis=0)
    x = np.repeat(base, rng.integers(1, 4, size=len(base)), axis=0).astype(np.float32)
    x = x[rng.permutation(len(x))]
    d, nb = cloud_ref.neighbor_distances(x, max_equal)
    assert np.array_equal(d, cloud_ref.neighbor_distances_literal(x, max_equal))
    assert ((d == 0) == (nb == -1)).all() and (d > 0).any()
    assert (d == 0).any() == (max_equal <= 1)           # up to three copies of a point: K = 4 reaches past them


def test_lattice_generator_is_the_brute_force_answer():
    for seed in (None, 5):
        x, d, nb = cloud_ref.lattice_case(6, 0.5, (-1.0, 2.0, 0.25), seed)
        bd, bnb = cloud_ref.neighbor_distances(x)
        assert np.array_equal(d, bd) and np.array_equal(nb, bnb)


def test_tiny_clouds_and_non_finite_points():
    assert cloud_ref.neighbor_distances(np.zeros((0, 3)))[0].shape == (0,)
    d, nb = cloud_ref.neighbor_distances(np.ones((1, 3)))
    assert d.tolist() == [0] and nb.tolist() == [-1]
    x = np.array([(0, 0, 0), (np.nan, 0, 0), (0, 3, 4), (np.inf, 1, 1)], np.float32)
    d, nb = cloud_ref.neighbor_distances(x)
    assert d.tolist() == [5, 0, 5, 0] and nb.tolist() == [2, -1, 0, -1]
