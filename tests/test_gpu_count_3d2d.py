"""GPU: sfmx_count_3d2d_matches (the candidate ranking of SfM.cpp:276-300 in one call) against the counts of
per-shot sfmx_find_3d2d_matches calls, exactly.  Fails without the feature: the entry point does not exist."""
import numpy as np
import pytest
import torch

from sfmx import scene
from sfmx.matching import DMATCH_DTYPE
import scene_cases
import sfm_cases

pytestmark = pytest.mark.gpu


def visible(pairs, m, off, active):
    """The match graph without the pairs a mask hides (what the per-shot call is given)."""
    if active is None:
        return pairs, m, off
    keep = [p for p in range(len(pairs)) if active[p]]
    lists = [m[off[p]:off[p + 1]] for p in keep]
    o = np.zeros(len(keep) + 1, np.int64)
    o[1:] = np.cumsum([len(x) for x in lists])
    return pairs[keep].reshape(-1, 2), (np.concatenate(lists) if lists else np.zeros(0, DMATCH_DTYPE)), o


def expected(kps, pairs, m, off, oo, osh, oxy, candidates, active=None):
    vp, vm, vo = visible(np.asarray(pairs, np.int32).reshape(-1, 2), m, off, active)
    return np.array([(scene.find_3d2d_matches(kps, vp, vm, vo, oo, osh, oxy, int(c))[0] >= 0).sum() for c in candidates],
                    np.int32).reshape(-1)


def device_counts(kps, pairs, m, off, oo, osh, oxy, candidates, active=None):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dk = [d(k) for k in kps]
    dm, doff, doo, dsh, dxy = d(m.view(np.uint8)), d(off), d(oo), d(osh), d(oxy)
    out = torch.full((max(len(candidates), 1),), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    scene.count_3d2d_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], pairs, dm.data_ptr(), doff.data_ptr(),
                                    doo.data_ptr(), len(oo) - 1, dsh.data_ptr(), dxy.data_ptr(), candidates, out.data_ptr(),
                                    pair_active=active)
    torch.cuda.synchronize()
    return out.cpu().numpy()[:len(candidates)]


@pytest.fixture(scope="module")
def synth_scene():
    case = scene_cases.scene_case(6, 1200, seed=5)
    return case, expected(*case, range(6))


def test_edge_case_every_candidate_list():
    """-0 / +0, NaN, a position that is no float, duplicate positions, a shot without a pair with the origins
    (3), two pairs joining the same shots (the first wins), an origin on the candidate itself, an empty list."""
    case = scene_cases.edge_case()
    full = expected(*case, range(4))
    assert full[0] == 4   # shot 0: the four matches the scene's docstring names
    for cand in ([], [0], [3], [2, 0], [0, 1, 2, 3], [3, 2, 1, 0]):
        got = scene.count_3d2d_matches(*case, cand)
        assert np.array_equal(got, full[cand]), (cand, got, full)
        assert np.array_equal(device_counts(*case, cand), full[cand]), cand


def test_synthetic_scene_host_and_device(synth_scene):
    case, full = synth_scene
    assert full.min() > 0
    for cand in ([4], [5, 0, 3], list(range(6))):
        assert np.array_equal(scene.count_3d2d_matches(*case, cand), full[cand]), cand
        assert np.array_equal(device_counts(*case, cand), full[cand]), cand
    assert scene.count_last_kernel_ms() > 0
    assert len(scene.count_3d2d_matches(*case, [])) == 0


def test_sfm_cloud_with_a_candidate_in_every_point_and_one_without_a_pair():
    sc = sfm_cases.scene(6, 400, graph=[(0, 1), (2, 1), (1, 3), (3, 0), (2, 0), (3, 2)], seed=21)   # shots 4, 5: no pair
    kps, pairs, m, off = sc["keypoints"], sc["pairs"], sc["matches"], sc["offsets"]
    # shot 1 is an origin shot of every point
    recs = [(kps[1][k].astype(np.float64), [(s, kps[s][np.flatnonzero(sc["point_id"][s] == p)[0]].astype(np.float64))
                                            for s in (0, 2) if p in sc["point_id"][s]]) for k, p in enumerate(sc["point_id"][1])]
    recs = [(a, b) for a, b in recs if b]
    oo = np.zeros(len(recs) + 1, np.int64)
    oo[1:] = np.cumsum([1 + len(b) for _, b in recs])
    osh = np.array([s for _, b in recs for s in [1] + [x[0] for x in b]], np.int32)
    oxy = np.array([xy for a, b in recs for xy in [a] + [x[1] for x in b]]).reshape(-1, 2)
    case = (kps, pairs, m, off, oo, osh, oxy)
    full = expected(*case, range(6))
    assert full[4] == 0 and full[5] == 0 and full[3] > 100 and full[1] > 0
    for cand in ([1], [4], [5, 4], [3, 1, 4], list(range(6))):
        assert np.array_equal(scene.count_3d2d_matches(*case, cand), full[cand]), cand
    assert np.array_equal(device_counts(*case, list(range(6))), full)


def test_first_pair_in_list_order_wins_and_a_mask_hides_it():
    """Pairs 0 (0,1) and 1 (1,0) join the same shots in both orientations with different lists."""
    rng = np.random.default_rng(4)
    kps = [rng.uniform(0, 400, (40, 2)).astype(np.float32) for _ in range(3)]
    pairs = np.array([[0, 1], [1, 0], [2, 1], [1, 2]], np.int32)
    lists = [[(q, q) for q in range(0, 10)],           # (0,1): keypoints 0..9 of shot 1 <- 0..9 of shot 0
             [(t, t) for t in range(5, 30)],           # (1,0): 5..29
             [(q, 39 - q) for q in range(20)],         # (2,1)
             [(q, q) for q in range(40)]]              # (1,2)
    off = np.zeros(5, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    m = np.array([(q, t, 0, 1.0) for x in lists for q, t in x], DMATCH_DTYPE)
    osh = np.array([1] * 40 + [0] * 40, np.int32)        # every keypoint of shots 1 and 0 is a record
    oxy = np.concatenate([kps[1], kps[0]]).astype(np.float64)
    oo = np.arange(81, dtype=np.int64)
    case = (kps, pairs, m, off, oo, osh, oxy)
    assert scene.count_3d2d_matches(*case, [0, 1, 2]).tolist() == [10, 10, 20]
    for active in ([1, 1, 1, 1], [0, 1, 1, 1], [0, 1, 0, 1], [1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, 1]):
        exp = expected(*case, [0, 1, 2], active)
        got = scene.count_3d2d_matches(*case, [0, 1, 2], pair_active=active)
        assert np.array_equal(got, exp), (active, got, exp)
        assert np.array_equal(device_counts(*case, [2, 1, 0], active), exp[::-1]), active
    assert scene.count_3d2d_matches(*case, [0, 1, 2], pair_active=[0, 1, 1, 1]).tolist() == [25, 25, 20]
    assert scene.count_3d2d_matches(*case, [2], pair_active=[1, 1, 0, 1]).tolist() == [40]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_record_counts_around_the_wave_and_the_block(synth_scene, n):
    (kps, pairs, m, off, oo, osh, oxy), _ = synth_scene
    assert len(osh) > 257
    sel = np.linspace(0, len(osh) - 1, n).astype(np.int64)   # spread over the cloud, one record per point
    case = (kps, pairs, m, off, np.arange(n + 1, dtype=np.int64), osh[sel], oxy[sel])
    exp = expected(*case, range(6))
    assert exp.sum() > 0
    assert np.array_equal(scene.count_3d2d_matches(*case, list(range(6))), exp)
    assert np.array_equal(device_counts(*case, [5, 2]), exp[[5, 2]])


def test_more_candidates_than_one_pass_of_the_kernel_holds():
    """1100 shots: the count kernel walks its candidates in passes of 1024."""
    n = 1100
    rng = np.random.default_rng(9)
    kps = [rng.uniform(0, 100, (4, 2)).astype(np.float32) for _ in range(n)]
    pairs = np.array([(0, s) if s % 2 else (s, 0) for s in range(1, n)], np.int32)
    lists = [[((q, 3 - q) if s % 2 else (3 - q, q)) for q in range(4) if (s >> q) & 1] for s in range(1, n)]
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    m = np.array([(q, t, 0, 1.0) for x in lists for q, t in x], DMATCH_DTYPE)
    osh = np.zeros(300, np.int32)                      # 300 records on shot 0, 75 at each of its keypoints
    oxy = kps[0][np.arange(300) % 4].astype(np.float64)
    case = (kps, pairs, m, off, np.arange(301, dtype=np.int64), osh, oxy)
    cand = list(range(n - 1, 0, -1))
    exp = np.array([75 * bin(s & 15).count("1") for s in cand], np.int32)
    got = scene.count_3d2d_matches(*case, cand)
    assert np.array_equal(got, exp)
    some = [1099, 1025, 1024, 1023, 16, 1]
    assert np.array_equal(expected(*case, some), np.array([75 * bin(s & 15).count("1") for s in some]))
    assert np.array_equal(device_counts(*case, cand), exp)


def test_invalid_arguments(synth_scene):
    (kps, pairs, m, off, oo, osh, oxy), _ = synth_scene
    for cand in ([6], [-1], [0, 6], [2, 2]):
        with pytest.raises(ValueError):
            scene.count_3d2d_matches(kps, pairs, m, off, oo, osh, oxy, cand)
    bad = oo.copy()
    bad[3] = bad[2] - 1
    with pytest.raises(ValueError):
        scene.count_3d2d_matches(kps, pairs, m, off, bad, osh, oxy, [0])
    bad = oo.copy()
    bad[0] = 1
    with pytest.raises(ValueError):
        scene.count_3d2d_matches(kps, pairs, m, off, bad, osh, oxy, [0])
    bad = off.copy()
    bad[2] = bad[1] - 1
    with pytest.raises(ValueError):
        scene.count_3d2d_matches(kps, pairs, m, bad, oo, osh, oxy, [0])
    bp = pairs.copy()
    bp[0, 1] = 6
    with pytest.raises(ValueError):
        scene.count_3d2d_matches(kps, bp, m, off, oo, osh, oxy, [0])
    bm = m.copy()
    bm["trainIdx"][0] = 10 ** 6
    with pytest.raises(ValueError):
        scene.count_3d2d_matches(kps, pairs, bm, off, oo, osh, oxy, [0, 1])
    with pytest.raises(ValueError):
        scene.count_3d2d_matches(kps, pairs, m, off, oo, osh, oxy, [0], pair_active=[1])
