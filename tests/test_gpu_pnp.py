"""GPU parity for the registration pose (SfM::findCameraPoseFrom3d2dMatch, SfM.cpp:453-489): the HIP kernels
(through the C ABI) against the numpy restatement tests/pnp_ref.py — as bit patterns for everything but the refit's
pose, which needs sin / cos / acos and is held to a tolerance derived from the restatement alone (the refit_tol fixture below).
The expected outputs of the cases are pinned in tests/golden/pnp_small.npz (tests/golden/make_pnp_golden.py); the
small sets are also recomputed live."""
import os

import numpy as np
import pytest
import torch

from sfmx import pnp, scene, triangulate
import pnp_cases
import pnp_ref
import scene_cases
import tri_cases
import tri_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("status", "ransac_pose", "mask", "n_inliers", "inlier_ratio", "refit_start")     # compared as bit patterns
QNAN = 0x7FF8000000000000
POSE_ERR = 2.19e-8       # the chain test's case in the restatement: refit pose against the planted pose
XYZ_ERR = 1.43e-6        # ... and tri_ref's points with that pose against the landmarks


def refit_sensitivity(case, golden):
    """The restatement's refit on the cases (every threshold) with each sin / cos / acos result moved by one ulp up
    or down (fixed seed): the largest change of a pose entry against the unperturbed golden pose."""
    rng = np.random.default_rng(20261020)

    def moved(f):
        return lambda x: float(np.nextafter(f(x), np.inf if rng.integers(2) else -np.inf))

    cams = [tri_ref.cam_params(K, d) for K, d in case["cameras"]]
    saved = pnp_ref._sin, pnp_ref._cos, pnp_ref._acos
    pnp_ref._sin, pnp_ref._cos, pnp_ref._acos = moved(saved[0]), moved(saved[1]), moved(saved[2])
    worst = 0.0
    try:
        for ti in range(len(pnp_cases.THRESHOLDS)):
            for s in np.flatnonzero(golden[f"t{ti}_refit_start"] >= 0):
                a, b = case["offsets"][s], case["offsets"][s + 1]
                cam = cams[case["shot_camera"][case["set_shot"][s]]]
                out = pnp_ref.refit(case["p3"][a:b].astype(np.float32), case["p2"][a:b].astype(np.float32),
                                    golden[f"t{ti}_mask"][a:b].astype(bool), cam, list(golden[f"t{ti}_ransac_pose"][s]))
                assert out is not None and out[1] == golden[f"t{ti}_refit_start"][s]
                worst = max(worst, float(np.abs(np.array(out[0]) - golden[f"t{ti}_pose"][s]).max()))
    finally:
        pnp_ref._sin, pnp_ref._cos, pnp_ref._acos = saved
    return worst


@pytest.fixture(scope="module")
def case():
    return pnp_cases.small_case()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pnp_small.npz"))


@pytest.fixture(scope="module")
def refit_tol(case, golden):
    """10 x the restatement's own sensitivity to one ulp in its libm results: not chosen from the GPU's output."""
    w = refit_sensitivity(case, golden)
    print("refit: largest pose change under +-1 ulp of sin / cos / acos", w, "-> tolerance", 10 * w)
    return 10 * w


def assert_pose_close(got, exp, tol, names=None):
    g, e = np.asarray(got["pose"]), np.asarray(exp["pose"])
    assert g.shape == e.shape and (np.isnan(g) == np.isnan(e)).all()
    d = np.nan_to_num(np.abs(g - e)).max(axis=1) if len(g) else np.zeros(0)
    print("refit pose: largest difference to the restatement", float(d.max()) if len(d) else 0.0, "tolerance", tol)
    assert (d <= tol).all(), (d.tolist(), names)
    five = np.asarray(exp["refit_start"]) < 0                   # no refit: the pose is the EPnP model, bit for bit
    assert g[five].tobytes() == e[five].tobytes()


@pytest.fixture(scope="module")
def host8(case):
    return pnp.register_poses(*pnp_cases.args(case), threshold=-8.0)


def assert_bits_equal(got, exp, names=None):
    for k in KEYS:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (k, g.shape, e.shape, g.dtype, e.dtype)
        if g.tobytes() != e.tobytes():
            rows = [i for i in range(len(e)) if g[i].tobytes() != e[i].tobytes()]
            raise AssertionError((k, len(rows), rows[:8], [names[i] for i in rows[:8]] if names and k != "mask" else None,
                                  g[rows[:2]], e[rows[:2]]))


@pytest.mark.parametrize("ti", range(len(pnp_cases.THRESHOLDS)))
def test_bit_parity_with_the_golden_restatement(case, golden, refit_tol, ti):
    got = pnp.register_poses(*pnp_cases.args(case), threshold=pnp_cases.THRESHOLDS[ti])
    assert_pose_close(got, {k: golden[f"t{ti}_{k}"] for k in ("pose", "refit_start")}, refit_tol, case["names"])
    rs = dict(zip(case["names"], got["refit_start"].tolist()))
    assert rs["planar"] == 1 and rs["len65"] == 0 and rs["len1025"] == 0 and rs["len5"] == -1 and rs["len4"] == -1
    print("threshold", pnp_cases.THRESHOLDS[ti], "status", got["status"].tolist(), "inliers", got["n_inliers"].tolist(),
          "kernel ms", pnp.last_kernel_ms())
    assert_bits_equal(got, {k: golden[f"t{ti}_{k}"] for k in KEYS}, case["names"])
    assert pnp.last_kernel_ms() > 0
    st = dict(zip(case["names"], got["status"].tolist()))
    assert st["len0"] == 0 and st["len3"] == 0 and st["len4"] == 2 and st["len5"] == 1 and st["repeated"] == 0
    assert st["len1025"] == 1 and st["nan"] == 1
    # the planar scene is posed through the three-control-point path: at 8 px every point is an inlier
    ip = case["names"].index("planar")
    assert st["planar"] == 1 and (got["n_inliers"][ip] == 80 or pnp_cases.THRESHOLDS[ti] == -1.0)
    bad = np.flatnonzero(got["status"] != 1)
    assert (got["ransac_pose"][bad].view(np.uint64) == QNAN).all() and (got["inlier_ratio"][bad] == -1.0).all()
    assert (got["pose"][bad].view(np.uint64) == QNAN).all()
    i5 = case["names"].index("len5")
    assert got["inlier_ratio"][i5] == 4 / 5 and got["n_inliers"][i5] == 5


def test_small_sets_recomputed_live(case, host8, refit_tol):
    sub = pnp_cases.subset(case, pnp_cases.SMALL)
    exp = pnp_ref.register_poses(*pnp_cases.args(sub), threshold=-8.0)
    got = pnp.register_poses(*pnp_cases.args(sub), threshold=-8.0)
    assert_bits_equal(got, exp, sub["names"])
    assert_pose_close(got, exp, refit_tol, sub["names"])
    for j, name in enumerate(sub["names"]):           # a set's result does not depend on the sets around it
        s = case["names"].index(name)
        assert got["ransac_pose"][j].tobytes() == host8["ransac_pose"][s].tobytes(), name
        assert got["n_inliers"][j] == host8["n_inliers"][s] and got["status"][j] == host8["status"][s], name


def test_a_set_does_not_depend_on_its_neighbours(case, host8):
    names = ["len1025", "nan", "len257", "len4", "len65", "noise", "len0"]     # another order, other neighbours
    sub = pnp_cases.subset(case, names)
    got = pnp.register_poses(*pnp_cases.args(sub), threshold=-8.0)
    o, so = case["offsets"], sub["offsets"]
    for j, name in enumerate(names):
        s = case["names"].index(name)
        for k in ("status", "pose", "ransac_pose", "n_inliers", "inlier_ratio", "refit_start"):
            assert got[k][j].tobytes() == host8[k][s].tobytes(), (name, k)
        assert got["mask"][so[j]:so[j + 1]].tobytes() == host8["mask"][o[s]:o[s + 1]].tobytes(), name


def test_device_inputs_equal_host_inputs_and_repeat(case, host8):
    p3, p2, off, ss, cams, sc, size = pnp_cases.args(case)
    d3, d2, do = torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda(), torch.from_numpy(off).cuda()
    for _ in range(2):
        dev = pnp.register_poses_device(d3.data_ptr(), d2.data_ptr(), do.data_ptr(), len(p3), ss, cams, sc, size,
                                        threshold=-8.0)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in dev.items()}
        assert_bits_equal(got, host8, case["names"])
        assert got["pose"].tobytes() == host8["pose"].tobytes()                  # the same kernels: the same bits
    again = pnp.register_poses(p3, p2, off, ss, cams, sc, size, threshold=-8.0)
    assert_bits_equal(again, host8, case["names"])
    assert again["pose"].tobytes() == host8["pose"].tobytes()
    # an empty device call: status 0, NaN poses and ratio -1, nothing launched
    dev = pnp.register_poses_device(d3.data_ptr(), d2.data_ptr(), torch.zeros(4, dtype=torch.int64).cuda().data_ptr(), 0,
                                    ss[:3], cams, sc, size)
    torch.cuda.synchronize()
    assert dev["status"].cpu().tolist() == [0, 0, 0] and dev["inlier_ratio"].cpu().tolist() == [-1.0] * 3
    assert (dev["ransac_pose"].cpu().numpy().view(np.uint64) == QNAN).all() and pnp.last_kernel_ms() == 0.0
    assert (dev["pose"].cpu().numpy().view(np.uint64) == QNAN).all() and dev["refit_start"].cpu().tolist() == [-1] * 3


def test_index_zero_quirk_and_float_rounding_on_the_device():
    X, px, cam, _, _ = pnp_cases.planted_scene(5, n=40)
    a = ([cam], [0], [(640, 480)])
    off = np.array([0, 40], np.int64)
    r = pnp.register_poses(X, px, off, [0], *a)
    assert r["n_inliers"][0] == 40 and r["inlier_ratio"][0] == 39 / 40          # point 0 is an inlier: not counted
    px2 = px.copy()
    px2[0] += 300.0
    r = pnp.register_poses(X, px2, off, [0], *a)
    assert r["mask"][0] == 0 and r["n_inliers"][0] == 39 and r["inlier_ratio"][0] == 39 / 40
    X2 = X * (1.0 + 1e-12)                                                         # not floats: rounded first
    assert (X2 != X).any() and (X2.astype(np.float32) == X.astype(np.float32)).all()
    r2 = pnp.register_poses(X2, px2, off, [0], *a)
    assert r2["ransac_pose"].tobytes() == r["ransac_pose"].tobytes()


def test_distinct_points_equal_the_restatement_on_the_scene():
    kps, pairs, m, off, oo, osh, oxy = scene_cases.scene_case()
    rng = np.random.default_rng(9)
    xyz = rng.uniform(-3, 3, (len(oo) - 1, 3))
    xyz[5] = xyz[2]                                    # equal coordinates at different point indices
    n_total = 0
    for shot in (2, 5):
        fk, _, fxy = scene.find_3d2d_matches(kps, pairs, m, off, oo, osh, oxy, shot)
        e3, e2 = pnp_ref.distinct_3d2d(xyz, oo, fk, fxy)
        g3, g2 = pnp.distinct_3d2d_points(xyz, oo, fk, fxy)
        assert g3.tobytes() == e3.tobytes() and g2.tobytes() == e2.tobytes(), shot
        assert 0 < len(e3) < int((fk >= 0).sum()) and pnp.distinct_last_kernel_ms() > 0     # something was dropped
        n_total += len(e3)
        # device inputs
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xyz, oo, fk, fxy)]
        d3, d2 = pnp.distinct_3d2d_points_device(t[0].data_ptr(), len(xyz), t[1].data_ptr(), t[2].data_ptr(),
                                                 t[3].data_ptr(), len(fk))
        torch.cuda.synchronize()
        assert d3.cpu().numpy().tobytes() == e3.tobytes() and d2.cpu().numpy().tobytes() == e2.tobytes()
    assert n_total > 100


def test_distinct_edge_cases():
    xyz = np.array([[1.0, 2, 3], [1.0, 2, 3], [-0.0, 0, 1], [0.0, 0, 1], [np.nan, 0, 1], [np.nan, 0, 1], [7.0, 8, 9]])
    oo = np.array([0, 2, 3, 4, 5, 6, 7, 8], np.int64)
    fk = np.array([4, 4, 9, 1, 1, 2, 2, -1], np.int32)
    fxy = np.array([[5, 6], [5, 6], [5, 6], [0, -0.0], [-0.0, 0], [1, 1], [1, 1], [np.nan, np.nan]], np.float32)
    e3, e2 = pnp_ref.distinct_3d2d(xyz, oo, fk, fxy)
    g3, g2 = pnp.distinct_3d2d_points(xyz, oo, fk, fxy)
    assert g3.tobytes() == e3.tobytes() and g2.tobytes() == e2.tobytes()
    # records 0, 1, 2 are one point (equal coordinates at two indices); -0 == +0; a NaN never equals
    assert len(e3) == 4 and np.isnan(e3[2:, 0]).all()


def test_chain_search_distinct_pose_triangulate(refit_tol):
    """f4 -> distinct -> f8 on a planted shot; the returned pose goes into triangulate_matches as shot_pose."""
    rng = np.random.default_rng(12)
    poses = tri_cases.arc_poses()
    n = 300
    land = tri_cases.landmarks(rng, n)
    cam_of = tri_cases.SHOT_CAMERA
    kps = [pnp_cases.observe(land, poses[s], cam_of[s], 0.0, rng).astype(np.float32) for s in range(3)]
    # shots 0 and 1 are registered: the cloud's points carry one origin record in each; shot 2 is the new one
    oo = 2 * np.arange(n + 1, dtype=np.int64)
    osh = np.tile([0, 1], n).astype(np.int32)
    oxy = np.stack([kps[0], kps[1]], axis=1).reshape(-1, 2).astype(np.float64)
    pairs = np.array([[0, 2], [1, 2]], np.int32)
    ids = np.arange(n)
    m, off = tri_cases._pack([np.stack([ids, ids], axis=1), np.stack([ids[::2], ids[::2]], axis=1)])
    fk, _, fxy = scene.find_3d2d_matches(kps, pairs, m, off, oo, osh, oxy, 2)
    xyz = land.astype(np.float64)
    p3, p2 = pnp.distinct_3d2d_points(xyz, oo, fk, fxy)
    e3, e2 = pnp_ref.distinct_3d2d(xyz, oo, fk, fxy)
    assert p3.tobytes() == e3.tobytes() and p2.tobytes() == e2.tobytes() and len(p3) == n     # both origins agree
    cams = tri_cases.CAMERAS
    got = pnp.register_poses(p3, p2, [0, n], [2], cams, cam_of[:3], pnp_cases.SHOT_SIZE[:3])
    exp = pnp_ref.register_poses(p3, p2, [0, n], [2], cams, cam_of[:3], pnp_cases.SHOT_SIZE[:3])
    assert_bits_equal(got, exp)
    assert got["status"][0] == 1 and got["n_inliers"][0] == n
    assert got["refit_start"][0] == 0 and np.abs(got["pose"][0] - exp["pose"][0]).max() <= refit_tol
    # Bounds: 10 x the restatement's own error on this case (POSE_ERR, XYZ_ERR below were measured with pnp_ref and
    # tri_ref on the CPU); the kernel's EPnP model equals the restatement's bit for bit, its refit within rounding.
    assert np.abs(got["pose"][0] - poses[2]).max() < 10 * POSE_ERR
    shot_pose = np.stack([poses[0], poses[1], got["pose"][0]])
    tri = triangulate.triangulate_matches(kps, cams, cam_of[:3], shot_pose, pairs[:1], m[:n], np.array([0, n], np.int64))
    assert len(tri["xyz"]) == n and np.abs(tri["xyz"] - xyz).max() < 10 * XYZ_ERR
