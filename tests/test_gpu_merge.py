"""GPU parity for the point-cloud merge (Scene::mergePointcloudElement3d2d, Scene.cpp:470-567, in the loop
of SfM.cpp:354-363): the hash join of csrc/merge.hip through the C ABI against the brute-force restatement
tests/merge_ref.py.  Every output array must be equal; merge_distance is compared as bit patterns (one
correctly rounded fp64 distance, no contraction, the same on both sides)."""
import numpy as np
import pytest
import torch

import sfmx
from sfmx import scene, triangulate
from sfmx.matching import DMATCH_DTYPE
import merge_cases
import merge_ref
import tri_cases

pytestmark = pytest.mark.gpu

KEYS = ("xyz", "origin_offsets", "origin_shot", "origin_xy", "target", "merge_distance")
KNOWN = merge_cases.known_cases()
INF = float("inf")


def assert_equal(got, exp):
    """Every array as bit patterns (coordinates and records are copied through, NaN payloads included)."""
    for k in KEYS:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.dtype == e.dtype and g.shape == e.shape, (k, g.dtype, e.dtype, g.shape, e.shape)
        if g.dtype == np.float64:
            g, e = g.view(np.uint64), e.view(np.uint64)
        bad = np.flatnonzero((g != e).reshape(-1))
        assert len(bad) == 0, (k, len(bad), bad[:8], g.reshape(-1)[bad[:8]], e.reshape(-1)[bad[:8]])


@pytest.fixture(scope="module")
def case():
    return merge_cases.scene_case()


@pytest.fixture(scope="module")
def expected(case):
    """The restatement on the scene case, computed once per (D, F, element range) and left unchanged."""
    cache = {}

    def get(D, F, a=0, b=None):
        b = len(case["new"][0]) if b is None else b
        if (D, F, a, b) not in cache:
            cache[D, F, a, b] = merge_ref.merge(*merge_cases.args(case, new=merge_cases.slice_new(case["new"], a, b)), D, F)
        return cache[D, F, a, b]
    return get


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answer(name):
    a, exp = KNOWN[name]
    assert_equal(scene.merge_pointcloud_3d2d(*a), exp)
    assert_equal(merge_ref.merge(*a), exp)


@pytest.mark.parametrize("F", merge_cases.F_SWEEP)
@pytest.mark.parametrize("D", merge_cases.D_SWEEP)
def test_scene_parity(case, expected, D, F):
    exp = expected(D, F)
    got = scene.merge_pointcloud_3d2d(*merge_cases.args(case), D, F)
    merged = got["merge_distance"] != -1.0
    print("D", D, "F", F, "merged", int(merged.sum()), "of", len(merged), "points", len(got["xyz"]))
    assert_equal(got, exp)
    assert scene.merge_last_kernel_ms() > 0


@pytest.mark.parametrize("F", merge_cases.F_SWEEP)
def test_scene_parity_every_point_near(case, expected, F):
    """D = inf: every cloud point is a candidate, the links alone decide."""
    k = merge_cases.INF_SLICE
    got = scene.merge_pointcloud_3d2d(*merge_cases.args(case, new=merge_cases.slice_new(case["new"], 0, k)), INF, F)
    assert_equal(got, expected(INF, F, 0, k))


@pytest.mark.parametrize("n_new", [1, 63, 64, 65, 257])
def test_element_counts_across_workgroup_boundaries(case, expected, n_new):
    """From element 300 on: the slice holds elements of two pairs, with links among them."""
    a = 300
    new = merge_cases.slice_new(case["new"], a, a + n_new)
    got = scene.merge_pointcloud_3d2d(*merge_cases.args(case, new=new), merge_cases.D_MID, 20.0)
    assert_equal(got, expected(merge_cases.D_MID, 20.0, a, a + n_new))


def _hot_case(n_hot=300):
    """n_hot cloud points holding the same record (a chain of equal keys in the record table) at distinct
    distances from the one element linked to it; the nearest is not the first."""
    kps, pairs, m, off = merge_cases._graph([(0, 1)], [[(0, 0, 1.0), (1, 1, 1.0)]])
    rng = np.random.default_rng(3)
    z = rng.permutation(n_hot) * 1e-4 + 1e-4
    pts = [((0.0, 0.0, float(zi)), [merge_cases._kp(0, 0)]) for zi in z]
    pts[17] = ((0.0, 0.0, float(z[200])), [merge_cases._kp(0, 0)])          # a tie between 17 and 200
    new = [((0.0, 0.0, 0.0), [merge_cases._kp(1, 0)]), ((0.0, 0.0, 0.0), [merge_cases._kp(1, 1)]),
           ((0.0, 0.0, 1e-5), [merge_cases._kp(1, 0), merge_cases._kp(3, 3)])]
    return (kps, pairs, m, off, *merge_cases._cloud(pts), *merge_cases._cloud(new))


def test_hot_key_chain():
    a = _hot_case()
    for D in (1.0, 0.02, 1e-4):
        exp = merge_ref.merge(*a, D, 20.0)
        assert_equal(scene.merge_pointcloud_3d2d(*a, D, 20.0), exp)
        if D == 0.02:
            assert exp["target"].tolist() == [exp["target"][0], 300, exp["target"][0]] and exp["target"][0] < 300


def test_keypoint_position_duplicated_across_indices():
    """SIFT emits one keypoint per orientation: several keypoint indices share a position.  The element's
    record equals keypoints 2, 3 and 4 of shot 1, and one DMatch through each of them joins it to a different
    cloud point; a fourth point is nearest but joined to nothing."""
    kps, pairs, m, off = merge_cases._graph([(0, 1)], [[(0, 2, 1.0), (1, 3, 1.0), (5, 4, 1.0), (6, 7, 1.0)]])
    kps[1][3] = kps[1][2]
    kps[1][4] = kps[1][2]
    kp = merge_cases._kp
    cloud = merge_cases._cloud([((0, 0, 0.004), [kp(0, 5)]), ((0, 0, 0.003), [kp(0, 1)]), ((0, 0, 0.009), [kp(0, 0)]),
                                ((0, 0, 0.001), [kp(0, 6)])])
    new = merge_cases._cloud([((0, 0, 0), [kp(1, 2)])])
    for D, want in ((0.02, 1), (0.0035, 1), (0.0025, 4)):
        exp = merge_ref.merge(kps, pairs, m, off, *cloud, *new, D, 20.0)
        assert exp["target"][0] == want
        assert_equal(scene.merge_pointcloud_3d2d(kps, pairs, m, off, *cloud, *new, D, 20.0), exp)


@pytest.mark.parametrize("F", [20.0, 0.5])
def test_split_equals_whole(case, expected, F):
    """Merging new[:k] and then new[k:] into the result equals one call: what was dynamic in the whole
    call (records and points added in the call) is static in the second half of the split."""
    D, n_new = merge_cases.D_MID, len(case["new"][0])
    whole = expected(D, F)
    for k in (1, n_new // 2, n_new - 1):
        first = scene.merge_pointcloud_3d2d(*merge_cases.args(case, new=merge_cases.slice_new(case["new"], 0, k)), D, F)
        second = scene.merge_pointcloud_3d2d(*merge_cases.args(case, new=merge_cases.slice_new(case["new"], k, n_new),
                                                               cloud=merge_cases.as_cloud(first)), D, F)
        joined = dict(second, target=np.concatenate([first["target"], second["target"]]),
                      merge_distance=np.concatenate([first["merge_distance"], second["merge_distance"]]))
        assert_equal(joined, whole)


def _device_call(case, D, F):
    kps, pairs, m, off = case["kps"], case["pairs"], case["matches"], case["offsets"]
    dk = [torch.from_numpy(k).cuda() for k in kps]
    dm = torch.from_numpy(m.view(np.uint8)).cuda()
    do = torch.from_numpy(off).cuda()
    clouds = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (*case["cloud"], *case["new"])]
    r = scene.merge_pointcloud_3d2d_device([t.data_ptr() for t in dk], [len(k) for k in kps], pairs, dm.data_ptr(),
                                           do.data_ptr(), *clouds, D, F)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_device_inputs_equal_host_inputs(case, expected):
    D = merge_cases.D_MID
    got = _device_call(case, D, 20.0)
    assert_equal(got, expected(D, 20.0))
    assert_equal(got, scene.merge_pointcloud_3d2d(*merge_cases.args(case), D, 20.0))
    none = dict(case, new=merge_cases.slice_new(case["new"], 0, 0))
    through = _device_call(none, D, 20.0)
    for k, a in zip(KEYS[:4], case["cloud"]):
        assert np.array_equal(through[k].reshape(-1), np.asarray(a).reshape(-1), equal_nan=True), k
    assert scene.merge_last_kernel_ms() == 0.0


def test_last_stats_match_the_restatement(case):
    """A merge is dynamic iff its winner qualified only through a record or a point added in the call."""
    st = {}
    exp = merge_ref.merge(*merge_cases.args(case), merge_cases.D_MID, 20.0, stats=st)
    assert_equal(scene.merge_pointcloud_3d2d(*merge_cases.args(case), merge_cases.D_MID, 20.0), exp)
    got = scene.merge_last_stats()
    assert got["merged_dynamic"] == st["dynamic"] > 0 and got["merged_static"] == st["merged"] - st["dynamic"] > 0
    assert got["links"] > 0
    # a NaN static first qualifier behind a finite same-call one, the nearest qualifier static: two static merges
    a, exp = KNOWN["nan_static_first_behind_dynamic"]
    st = {}
    assert_equal(merge_ref.merge(*a, stats=st), exp)
    assert_equal(scene.merge_pointcloud_3d2d(*a), exp)
    got = scene.merge_last_stats()
    assert (got["merged_static"], got["merged_dynamic"], got["links"]) == (2, 0, 1) and st["dynamic"] == 0


def test_repeated_call_is_bitwise_equal(case):
    a = merge_cases.args(case)
    r1 = scene.merge_pointcloud_3d2d(*a, merge_cases.D_MID, 20.0)
    r2 = scene.merge_pointcloud_3d2d(*a, merge_cases.D_MID, 20.0)
    for k in KEYS:
        assert r1[k].tobytes() == r2[k].tobytes(), k


def test_chain_triangulate_merge_find_ba():
    """triangulate_matches -> merge_pointcloud_3d2d -> find_3d2d_matches / ba_observations_from_origins,
    against the same chain with the merge done by the restatement; tracks of three and more records form."""
    rng = np.random.default_rng(11)
    poses = tri_cases.arc_poses()
    land = tri_cases.landmarks(rng)
    kps, slot = tri_cases.observe(land, poses, 0.0, rng)
    prs = [(0, 1), (1, 2), (0, 2), (2, 3), (1, 3)]
    js = [rng.choice(300, 150, replace=False) for _ in prs]
    m = np.zeros(150 * len(prs), DMATCH_DTYPE)
    m["queryIdx"] = np.concatenate([slot[L][j] for (L, _), j in zip(prs, js)])
    m["trainIdx"] = np.concatenate([slot[R][j] for (_, R), j in zip(prs, js)])
    m["distance"] = 1.0
    off = 150 * np.arange(len(prs) + 1, dtype=np.int64)
    pairs = np.array(prs, np.int32)
    tri = triangulate.triangulate_matches(kps, tri_cases.CAMERAS, tri_cases.SHOT_CAMERA, poses, pairs, m, off)
    empty = (np.zeros((0, 3)), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2)))
    new = (tri["xyz"], tri["origin_offsets"], tri["origin_shot"], tri["origin_xy"])
    got = sfmx.merge_pointcloud_3d2d(kps, pairs, m, off, *empty, *new)
    exp = merge_ref.merge(kps, pairs, m, off, *empty, *new)
    assert_equal(got, exp)
    assert np.diff(got["origin_offsets"]).max() >= 3 and len(got["xyz"]) < tri["n_points"]
    for cloud in (got, exp):
        assert cloud["origin_offsets"][-1] == len(cloud["origin_shot"])
    obs_g = scene.ba_observations_from_origins(got["origin_offsets"], got["origin_shot"], got["origin_xy"], len(kps))
    obs_e = scene.ba_observations_from_origins(exp["origin_offsets"], exp["origin_shot"], exp["origin_xy"], len(kps))
    for k in obs_e:
        assert np.array_equal(obs_g[k], obs_e[k]), k
    assert np.bincount(obs_g["obs_point"]).max() >= 3
    # a new shot: the tracks are found from it through any of their records
    fg = scene.find_3d2d_matches(kps, pairs, m, off, got["origin_offsets"], got["origin_shot"], got["origin_xy"], 3)
    fe = scene.find_3d2d_matches(kps, pairs, m, off, exp["origin_offsets"], exp["origin_shot"], exp["origin_xy"], 3)
    for g, e in zip(fg, fe):
        assert np.array_equal(g, e, equal_nan=True)
    assert (fg[0] >= 0).sum() > 50
