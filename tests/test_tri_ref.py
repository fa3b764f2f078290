"""CPU: the numpy restatement of SfM::triangulateMatch (tests/tri_ref.py), the specification the HIP
kernels are compared with bit for bit (tests/test_gpu_triangulate.py), checked on its own: against an
independent SVD, on an exact scene, on its NaN / W == 0 rules, and pinned to a committed golden file."""
import numpy as np
import pytest

import fixtures
import tri_cases
import tri_ref

THRESHOLDS = (10.0, 0.5, 0.0)


@pytest.fixture(scope="module")
def case():
    return tri_cases.small_case()


@pytest.fixture(scope="module")
def ref(case):
    return {t: tri_ref.triangulate_matches(*tri_cases.args(case), t) for t in THRESHOLDS}


def _ordered(f):
    """float32 bit patterns as integers that ascend with the value (ulp distance = difference)."""
    i = f.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def test_case_shape(case, ref):
    off, r = case["offsets"], ref[10.0]
    lengths = np.diff(off)
    assert set(tri_cases.MAIN_LENGTHS) <= set(lengths.tolist()) and (lengths[7:7 + tri_cases.N_SHORT] < 40).all()
    assert 2000 < off[-1] <= 5000 and off[-1] > 8 * 256             # several 256-match blocks
    inner = off[1:-1]
    assert np.count_nonzero(inner % 256) >= 40                        # blocks straddle pair boundaries
    kept = np.diff(r["point_offsets"])
    e = case["edge"]
    assert kept[e["all_fail"]] == 0 and lengths[e["all_fail"]] == 40
    assert kept[e["all_pass"]] == lengths[e["all_pass"]] == 50
    o = case["ordinary"]
    n_ord, k_ord = int(off[o[-1] + 1]), int(r["point_offsets"][o[-1] + 1])
    assert 0.8 * n_ord < k_ord < 0.95 * n_ord                         # every 8th match is an outlier
    assert r["sweeps"][:n_ord].max() <= 8                             # well conditioned: a few sweeps
    assert r["n_points"] > ref[0.5]["n_points"] > ref[0.0]["n_points"] > 0


def test_agrees_with_svd_dlt(case):
    """An independent DLT (numpy.linalg.svd of the same 4x4 system, then a float division) agrees within
    4 float ulps per coordinate on the well-conditioned pairs (measured: 1; the reciprocal-then-multiply
    of convertPointsFromHomogeneous and one rounding flip of a homogeneous coordinate are the margin)."""
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    cams = [tri_ref.cam_params(*c) for c in cams]
    worst = 0
    for p in case["ordinary"]:
        a, b = off[p], off[p + 1]
        if a == b:
            continue
        L, R = pairs[p]
        l, r = kps[L][m["queryIdx"][a:b]], kps[R][m["trainIdx"][a:b]]
        X, Y, Z, eL, eR, _ = tri_ref.triangulate_pair(l, r, poses[L], poses[R], cams[sc[L]], cams[sc[R]])
        keep = ~((eL > 10.0) | (eR > 10.0))                            # outlier matches are not well conditioned
        A = tri_ref.dlt_matrix(poses[L], poses[R], *tri_ref.undistort(l, cams[sc[L]]), *tri_ref.undistort(r, cams[sc[R]]))
        h = np.linalg.svd(A)[2][:, 3, :].astype(np.float32)
        exp = h[:, :3] / h[:, 3:]
        got = np.stack([X, Y, Z], axis=1)
        ulps = np.abs(_ordered(got) - _ordered(exp))[keep]
        worst = max(worst, int(ulps.max(initial=0)))
    print("worst ulp distance", worst)
    assert worst <= 4


def test_exact_scene_recovers_landmarks():
    c = tri_cases.exact_case()
    r = tri_ref.triangulate_matches(*tri_cases.args(c))
    assert r["n_points"] == len(c["land"]) and np.array_equal(r["match"], np.arange(len(c["land"])))
    rel = np.abs(r["xyz"] - c["land"]).max(axis=1) / np.abs(c["land"]).max(axis=1)
    print("worst relative error", rel.max(), "worst reprojection error", r["err"].max())
    assert rel.max() < 1e-4 and r["err"].max() < 1e-3


def test_nan_keypoint_is_kept(case, ref):
    p = case["edge"]["same_pose"]
    a, b = case["offsets"][p], case["offsets"][p + 1]
    for t in THRESHOLDS:
        r = ref[t]
        nan = np.isnan(r["err"][a:b]).all(axis=1)
        assert nan.sum() >= 4
        kept = np.isin(np.arange(a, b), r["match"])
        assert kept[nan].all()                                         # NaN > max is false: the reference keeps it
        sel = np.isin(r["match"], np.arange(a, b)[nan])
        assert np.isnan(r["xyz"][sel]).all()
        assert np.all(r["xyz"][sel].view(np.uint64) == np.float64(np.nan).view(np.uint64))   # canonical quiet NaN
    assert np.isnan(ref[0.0]["origin_xy"]).any()


def test_w_zero_takes_scale_one():
    h = np.array([[1.5, -2.0, 3.0, 0.0], [1.5, -2.0, 3.0, -0.0], [1.5, -2.0, 3.0, 2.0]], np.float32)
    X, Y, Z = tri_ref.from_homogeneous(h)
    assert np.array_equal(np.stack([X, Y, Z], axis=1), np.array([[1.5, -2, 3], [1.5, -2, 3], [0.75, -1, 1.5]], np.float32))
    assert X.dtype == np.float32


def test_jacobi_null_vector_of_a_known_system():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((50, 4, 4))
    h, sweeps = tri_ref.jacobi_null(A)
    s = np.linalg.svd(A)
    exp = s[2][:, 3, :]
    exp = exp * np.sign(np.sum(exp * h, axis=1, keepdims=True))
    assert np.abs(h - exp).max() < 1e-9 and sweeps.max() <= 12
    assert np.abs(np.einsum("nij,nj->ni", A, h)).max() <= 1.0001 * s[1][:, 3].max() + 1e-12


def test_pinned_to_golden(case, ref):
    """tests/golden/triangulate_small.npz holds the restatement's outputs on the case (threshold 10 in
    full; for 0.5 and 0 the offsets and kept match indices, the rest follows from the per-match arrays)."""
    g = fixtures.load("triangulate_small")
    r = ref[10.0]
    for k, view in (("point_offsets", np.int64), ("xyz", np.uint64), ("match", np.int64), ("origin_shot", np.int32),
                    ("origin_xy", np.uint64), ("err", np.uint64)):
        assert np.array_equal(np.ascontiguousarray(r[k]).view(view), g[k].view(view)), k
    for t, tag in ((0.5, "t05"), (0.0, "t0")):
        assert np.array_equal(ref[t]["point_offsets"], g[f"point_offsets_{tag}"]), t
        assert np.array_equal(ref[t]["match"], g[f"match_{tag}"]), t
        sel = g[f"match_{tag}"]
        assert np.array_equal(ref[t]["xyz"].view(np.uint64), r["xyz32"][sel].astype(np.float64).view(np.uint64))
