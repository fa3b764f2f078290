"""GPU parity for the triangulation step (SfM::triangulateMatch, SfM.cpp:383-451): the HIP kernels
(through the C ABI) against the numpy restatement tests/tri_ref.py, as bit patterns: both evaluate the
same correctly rounded IEEE operations in the same order, with no FMA contraction and no libm."""
import numpy as np
import pytest
import torch

import sfmx
from sfmx import scene, triangulate
import tri_cases
import tri_ref

pytestmark = pytest.mark.gpu

BITS = (("point_offsets", np.int64), ("xyz", np.uint64), ("match", np.int64), ("origin_offsets", np.int64),
        ("origin_shot", np.int32), ("origin_xy", np.uint64), ("err", np.uint64))


@pytest.fixture(scope="module")
def case():
    return tri_cases.small_case()


@pytest.fixture(scope="module")
def host10(case):
    return triangulate.triangulate_matches(*tri_cases.args(case))


def assert_bits_equal(got, exp, keys=BITS):
    assert got["n_points"] == exp["n_points"], (got["n_points"], exp["n_points"])
    for k, view in keys:
        g, e = np.ascontiguousarray(got[k]).reshape(-1).view(view), np.ascontiguousarray(exp[k]).reshape(-1).view(view)
        assert g.shape == e.shape, (k, g.shape, e.shape)
        bad = np.flatnonzero(g != e)
        assert len(bad) == 0, (k, len(bad), bad[:8], g[bad[:8]], e[bad[:8]])


@pytest.mark.parametrize("max_err", [10.0, 0.5, 0.0])
def test_bit_parity(case, max_err):
    exp = tri_ref.triangulate_matches(*tri_cases.args(case), max_err)
    got = triangulate.triangulate_matches(*tri_cases.args(case), max_err)
    print("matches", len(case["matches"]), "kept", got["n_points"], "NaN errors", int(np.isnan(got["err"]).any(axis=1).sum()))
    assert_bits_equal(got, exp)
    assert triangulate.last_kernel_ms() > 0


def test_exact_scene():
    c = tri_cases.exact_case()
    assert_bits_equal(triangulate.triangulate_matches(*tri_cases.args(c)), tri_ref.triangulate_matches(*tri_cases.args(c)))


def test_list_longer_than_one_scan_chunk():
    """The block-count scan walks the counts in chunks of 1024 blocks (262144 matches): 270 copies of a
    1000-match pair cross that chunk; matches are independent, so the expected output is the tiled one."""
    c = tri_cases.small_case()
    p = 6
    a, b = c["offsets"][p], c["offsets"][p + 1]
    reps, m1 = 270, c["matches"][a:b]
    one = tri_ref.triangulate_matches(c["kps"], c["cameras"], c["shot_camera"], c["poses"], c["pairs"][p:p + 1], m1,
                                      np.array([0, b - a], np.int64), 0.5)
    k, n1 = one["n_points"], b - a
    assert 0 < k < n1 and reps * n1 > 262144
    got = triangulate.triangulate_matches(c["kps"], c["cameras"], c["shot_camera"], c["poses"],
                                          np.repeat(c["pairs"][p:p + 1], reps, axis=0), np.tile(m1, reps),
                                          n1 * np.arange(reps + 1, dtype=np.int64), 0.5)
    exp = dict(n_points=reps * k, point_offsets=k * np.arange(reps + 1, dtype=np.int64), xyz=np.tile(one["xyz"], (reps, 1)),
               match=(one["match"][None, :] + n1 * np.arange(reps)[:, None]).reshape(-1),
               origin_offsets=2 * np.arange(reps * k + 1, dtype=np.int64), origin_shot=np.tile(one["origin_shot"], reps),
               origin_xy=np.tile(one["origin_xy"], (reps, 1)), err=np.tile(one["err"], (reps, 1)))
    assert_bits_equal(got, exp)


def test_device_inputs_equal_host_inputs(case, host10):
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    dk = [torch.from_numpy(k).cuda() for k in kps]
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    do = torch.from_numpy(off).cuda()
    dev = triangulate.triangulate_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, poses, pairs,
                                                 dm.data_ptr(), do.data_ptr(), len(m), with_err=True)
    torch.cuda.synchronize()
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in dev.items()}
    assert_bits_equal(got, host10)
    noerr = triangulate.triangulate_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, poses,
                                                   pairs, dm.data_ptr(), do.data_ptr(), len(m))
    assert "err" not in noerr and torch.equal(noerr["xyz"].view(torch.int64), dev["xyz"].view(torch.int64))


def test_origins_chain_into_scene_and_ba(case, host10):
    """The returned origin CSR goes unchanged into find_3d2d_matches and ba_observations_from_origins."""
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    r = host10
    n = r["n_points"]
    sel = r["match"]
    exp_xy = np.empty((2 * n, 2), np.float32)
    shots = np.repeat(pairs, np.diff(off), axis=0)[sel]
    exp_xy[0::2] = np.stack([kps[L][q] for L, q in zip(shots[:, 0], m["queryIdx"][sel])])
    exp_xy[1::2] = np.stack([kps[R][t] for R, t in zip(shots[:, 1], m["trainIdx"][sel])])
    assert np.array_equal(r["origin_shot"], shots.reshape(-1))
    obs = scene.ba_observations_from_origins(r["origin_offsets"], r["origin_shot"], r["origin_xy"], len(kps))
    assert len(obs["obs_point"]) == 2 * n and np.array_equal(obs["obs_point"], np.repeat(np.arange(n), 2))
    assert np.array_equal(obs["obs_xy"], exp_xy.astype(np.float64), equal_nan=True)
    assert np.array_equal(obs["shot_of_pose"][obs["obs_cam"]], r["origin_shot"])
    for shot in (0, 3):
        gk, gp, gxy = scene.find_3d2d_matches(kps, pairs, m, off, r["origin_offsets"], r["origin_shot"], r["origin_xy"], shot)
        hit = gk >= 0
        assert len(gk) == 2 * n and hit.sum() > 100
        assert not hit[r["origin_shot"] == shot].any()                 # a shot is not matched against itself
        assert np.array_equal(gxy[hit], kps[shot][gk[hit]])
        # every hit joins the origin's keypoint through a match of the pair used
        for i in np.flatnonzero(hit)[:200]:
            pr, o = gp[i], r["origin_shot"][i]
            lst = m[off[pr]:off[pr + 1]]
            oside, sside = ("queryIdx", "trainIdx") if pairs[pr][0] == o else ("trainIdx", "queryIdx")
            assert set(pairs[pr]) == {o, shot}
            assert ((kps[o][lst[oside]].astype(np.float64) == r["origin_xy"][i]).all(axis=1) & (lst[sside] == gk[i])).any()


def test_scene_mirror_equals_array_call(case, host10):
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    sc_ = sfmx.Scene([sfmx.Shot(f"img{i}", None, k, (640, 480)) for i, k in enumerate(kps)])
    sms = [sfmx.ShotMatches(int(l), int(r), m[off[p]:off[p + 1]]) for p, (l, r) in enumerate(pairs)]
    per_shot = [cams[c] for c in sc]
    got = triangulate.triangulateMatch(sc_, sms, per_shot, poses)
    assert_bits_equal(got, host10)
    p = 6
    one = triangulate.triangulateMatch(sc_, sms[p], per_shot, poses, maxReprojectionError=10.0)
    a, b = host10["point_offsets"][p], host10["point_offsets"][p + 1]
    assert one["n_points"] == b - a and np.array_equal(one["xyz"].view(np.uint64), host10["xyz"][a:b].view(np.uint64))
    assert np.array_equal(one["match"], host10["match"][a:b] - off[p])


def test_bad_index_rejected_host_and_device(case):
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    for field, value in (("trainIdx", 10 ** 6), ("queryIdx", -1)):
        bad = m.copy()
        bad[field][1500] = value
        with pytest.raises(ValueError):
            triangulate.triangulate_matches(kps, cams, sc, poses, pairs, bad, off)
        dk = [torch.from_numpy(k).cuda() for k in kps]
        dm = torch.from_numpy(bad.view(np.uint8)).cuda()
        do = torch.from_numpy(off).cuda()
        with pytest.raises(ValueError):
            triangulate.triangulate_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, poses, pairs,
                                                   dm.data_ptr(), do.data_ptr(), len(bad))


def test_empty_inputs_launch_nothing(case, host10):
    kps, cams, sc, poses, pairs, m, off = tri_cases.args(case)
    none = np.zeros((0, 2), np.int32)
    for prs in (none, pairs[:5]):
        zoff = np.zeros(len(prs) + 1, np.int64)
        r = triangulate.triangulate_matches(kps, cams, sc, poses, prs, m[:0], zoff)
        assert r["n_points"] == 0 and not r["point_offsets"].any() and len(r["point_offsets"]) == len(prs) + 1
        assert r["xyz"].shape == (0, 3) and r["origin_offsets"].tolist() == [0] and triangulate.last_kernel_ms() == 0.0
        dk = [torch.from_numpy(k).cuda() for k in kps]
        do = torch.from_numpy(zoff).cuda()
        d = triangulate.triangulate_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, poses, prs,
                                                   0, do.data_ptr(), 0)
        assert d["n_points"] == 0 and not d["point_offsets"].cpu().numpy().any() and len(d["xyz"]) == 0
        assert triangulate.last_kernel_ms() == 0.0
