"""GPU parity for the relative-pose step (SfM::findCameraPoseFromMatch, SfM.cpp:491-540): the HIP kernels
(through the C ABI) against the numpy restatement tests/pose_ref.py, as bit patterns.  The expected outputs of
the cases are pinned in tests/golden/pose_small.npz (tests/golden/make_pose_golden.py); the small pairs are also
recomputed live."""
import os

import numpy as np
import pytest
import torch

from sfmx import pose, triangulate
from sfmx.matching import DMATCH_DTYPE
import pose_cases
import pose_ref
import tri_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("status", "E", "pose", "mask", "n_ransac_inliers", "n_inliers", "matches", "pair_offsets")


@pytest.fixture(scope="module")
def case():
    return pose_cases.small_case()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pose_small.npz"))


@pytest.fixture(scope="module")
def host1(case):
    return pose.relative_poses(*pose_cases.args(case), threshold=-1.0)


def assert_bits_equal(got, exp, names=None):
    for k in KEYS:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (k, g.shape, e.shape, g.dtype, e.dtype)
        if g.tobytes() != e.tobytes():
            rows = [i for i in range(len(e)) if g[i].tobytes() != e[i].tobytes()]
            raise AssertionError((k, len(rows), rows[:8], [names[i] for i in rows[:8]] if names and k in ("E", "pose", "status") else None,
                                  g[rows[:2]], e[rows[:2]]))


@pytest.mark.parametrize("ti", range(len(pose_cases.THRESHOLDS)))
def test_bit_parity_with_the_golden_restatement(case, golden, ti):
    got = pose.relative_poses(*pose_cases.args(case), threshold=pose_cases.THRESHOLDS[ti])
    print("threshold", pose_cases.THRESHOLDS[ti], "status", got["status"].tolist(), "inliers", got["n_inliers"].tolist(),
          "kernel ms", pose.last_kernel_ms())
    assert_bits_equal(got, {k: golden[f"t{ti}_{k}"] for k in KEYS}, case["names"])
    assert pose.last_kernel_ms() > 0
    st = got["status"]
    assert st[case["names"].index("len4")] == 0 and st[case["names"].index("repeated")] == 0 and st.sum() >= 9
    bad = np.flatnonzero(st == 0)
    assert (got["E"][bad].view(np.uint64) == 0x7FF8000000000000).all() and (got["pose"][bad].view(np.uint64) == 0x7FF8000000000000).all()


def test_noise_pair_with_64_iterations(golden):
    got = pose.relative_poses(*pose_cases.args(pose_cases.noise_case()), threshold=-1.0, max_iters=pose_cases.NOISE_MAX_ITERS)
    assert_bits_equal(got, {k: golden[f"noise_{k}"] for k in KEYS})


def test_small_pairs_recomputed_live(case, host1):
    idx = [case["names"].index(n) for n in pose_cases.SMALL]
    off = case["offsets"]
    lists = [case["matches"][off[p]:off[p + 1]] for p in idx]
    m = np.concatenate(lists)
    o = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    a = (case["kps"], case["cameras"], case["shot_camera"], case["shot_size"], case["pairs"][idx], m, o)
    exp = pose_ref.relative_poses(*a, threshold=-1.0)
    got = pose.relative_poses(*a, threshold=-1.0)
    assert_bits_equal(got, exp)
    for j, p in enumerate(idx):                       # a pair's result does not depend on the pairs around it
        assert got["E"][j].tobytes() == host1["E"][p].tobytes() and got["n_inliers"][j] == host1["n_inliers"][p]


def test_device_inputs_equal_host_inputs_and_repeat(case, host1):
    kps, cams, sc, size, pairs, m, off = pose_cases.args(case)
    dk = [torch.from_numpy(k).cuda() for k in kps]
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    do = torch.from_numpy(off).cuda()
    for _ in range(2):
        dev = pose.relative_poses_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, size, pairs,
                                         dm.data_ptr(), do.data_ptr(), len(m), threshold=-1.0)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in dev.items()}
        total = int(got["pair_offsets"][-1])
        got["matches"] = got["matches"][:total].reshape(-1).view(DMATCH_DTYPE)
        assert_bits_equal(got, host1)
    again = pose.relative_poses(kps, cams, sc, size, pairs, m, off, threshold=-1.0)
    assert_bits_equal(again, host1)
    # an empty device call: status 0 and NaN everywhere, nothing launched
    dev = pose.relative_poses_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, size, pairs[:3],
                                     dm.data_ptr(), torch.zeros(4, dtype=torch.int64).cuda().data_ptr(), 0)
    torch.cuda.synchronize()
    assert dev["status"].cpu().tolist() == [0, 0, 0] and dev["pair_offsets"].cpu().tolist() == [0, 0, 0, 0]
    assert (dev["pose"].cpu().numpy().view(np.uint64) == 0x7FF8000000000000).all() and pose.last_kernel_ms() == 0.0


def test_bad_indices_are_reported_from_both_sides(case):
    kps, cams, sc, size, pairs, m, off = pose_cases.args(case)
    p = case["names"].index("len64")
    for field, shot in (("queryIdx", pairs[p][0]), ("trainIdx", pairs[p][1])):
        for v in (-1, len(kps[shot])):
            bad = m.copy()
            bad[field][off[p] + 9] = v
            with pytest.raises(ValueError, match="keypoints"):
                pose.relative_poses(kps, cams, sc, size, pairs, bad, off)
            dk = [torch.from_numpy(k).cuda() for k in kps]
            dm = torch.from_numpy(bad.view(np.uint8)).cuda()
            do = torch.from_numpy(off).cuda()
            with pytest.raises(ValueError, match="keypoints"):
                pose.relative_poses_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, size, pairs,
                                           dm.data_ptr(), do.data_ptr(), len(m))


def test_scene_mirror_equals_array_call(case, golden):
    import sfmx
    per_shot = [case["cameras"][c] for c in case["shot_camera"]]
    sc = sfmx.Scene([sfmx.Shot(f"img{i}", None, k, tuple(int(v) for v in case["shot_size"][i])) for i, k in enumerate(case["kps"])])
    off = case["offsets"]
    for ti, thr in ((0, -1.0), (2, 0.002)):                 # the positive threshold goes through the shots' sizes
        p = case["names"].index("len65")
        sm = sfmx.ShotMatches(int(case["pairs"][p][0]), int(case["pairs"][p][1]), case["matches"][off[p]:off[p + 1]])
        P, inl = sfmx.findCameraPoseFromMatch(sc, sm, thr, cameras=per_shot)
        a, b = golden[f"t{ti}_pair_offsets"][p], golden[f"t{ti}_pair_offsets"][p + 1]
        assert P.shape == (3, 4) and P.tobytes() == golden[f"t{ti}_pose"][p].tobytes()
        assert inl.tobytes() == golden[f"t{ti}_matches"][a:b].tobytes()
    for i, sh in enumerate(sc.getShots()):
        sh.camera = per_shot[i]
    p = case["names"].index("len4")
    with pytest.raises(RuntimeError, match="no pose"):
        sfmx.findCameraPoseFromMatch(sc, sfmx.ShotMatches(int(case["pairs"][p][0]), int(case["pairs"][p][1]),
                                                          case["matches"][off[p]:off[p + 1]]))


def test_chain_into_triangulation(case, golden):
    """The call's pose (left shot at the identity) and inlier list go straight into sfmx_triangulate_matches: on
    the 30 %-outlier pair the kept points are exactly those of the numpy chain pose_ref -> tri_ref."""
    p = case["names"].index(pose_cases.OUTLIER_PAIR)
    L, R = case["pairs"][p]
    a, b = case["offsets"][p], case["offsets"][p + 1]
    one = (case["kps"], case["cameras"], case["shot_camera"], case["shot_size"], case["pairs"][p:p + 1],
           case["matches"][a:b], np.array([0, b - a], np.int64))
    got = pose.relative_poses(*one, threshold=-1.0)
    assert got["status"][0] == 1 and 0.5 * (b - a) < got["n_inliers"][0] < 0.8 * (b - a)

    def poses_with(right):
        P = np.zeros((len(case["kps"]), 12))
        P[:, [0, 5, 10]] = 1.0
        P[R] = right
        return P

    tri = triangulate.triangulate_matches(case["kps"], case["cameras"], case["shot_camera"], poses_with(got["pose"][0]),
                                          case["pairs"][p:p + 1], got["matches"], got["pair_offsets"])
    ga, gb = golden["t0_pair_offsets"][p], golden["t0_pair_offsets"][p + 1]
    exp = tri_ref.triangulate_matches(case["kps"], case["cameras"], case["shot_camera"], poses_with(golden["t0_pose"][p]),
                                      case["pairs"][p:p + 1], golden["t0_matches"][ga:gb], np.array([0, gb - ga], np.int64))
    assert tri["n_points"] == exp["n_points"] > 0.9 * got["n_inliers"][0]
    for k in ("point_offsets", "xyz", "match", "origin_shot", "origin_xy", "err"):
        assert np.ascontiguousarray(tri[k]).tobytes() == np.ascontiguousarray(exp[k]).tobytes(), k
    assert L != R
