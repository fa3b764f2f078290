"""GPU: the merge's device resolution and dedupe (csrc/merge.hip: resolve rounds, group walk, three-launch scans,
device-mode input check) against tests/merge_ref.py and against the host resolution the same library falls back to.
Every output array must be equal, merge_distance as bit patterns; the path taken is read from
scene.merge_last_path()."""
import numpy as np
import pytest
import torch

from sfmx import ba, scene, sfm
import merge_cases
import merge_ref
import sfm_cases

pytestmark = pytest.mark.gpu

KEYS = ("xyz", "origin_offsets", "origin_shot", "origin_xy", "target", "merge_distance")
KNOWN = merge_cases.known_cases()
INF = float("inf")
SETTINGS = (0, -1, 1)   # the default cap, the host resolution always, a cap of one round
SCAN_BLOCK = 256        # csrc/merge.hip: values one block scans; the top level hands each of its SCAN_BLOCK threads
                        # one block sum up to SCAN_BLOCK * SCAN_BLOCK values and a run of several beyond


def assert_equal(got, exp):
    """Every array as bit patterns (coordinates and records are copied through, NaN payloads included)."""
    for k in KEYS:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.dtype == e.dtype and g.shape == e.shape, (k, g.dtype, e.dtype, g.shape, e.shape)
        if g.dtype == np.float64:
            g, e = g.view(np.uint64), e.view(np.uint64)
        bad = np.flatnonzero((g != e).reshape(-1))
        assert len(bad) == 0, (k, len(bad), bad[:8], g.reshape(-1)[bad[:8]], e.reshape(-1)[bad[:8]])


@pytest.fixture(autouse=True)
def default_cap_afterwards():
    yield
    scene.merge_set_max_rounds(0)


@pytest.fixture(scope="module")
def case():
    return merge_cases.scene_case()


@pytest.fixture(scope="module")
def head(case):
    """The scene case's first 60 elements, and the restatement's answer at D_MID, computed once."""
    c = dict(case, new=merge_cases.slice_new(case["new"], 0, 60))
    return c, merge_ref.merge(*merge_cases.args(c), merge_cases.D_MID, 20.0)


class DeviceGraph:
    """The match graph of a case resident on the device, for merge_pointcloud_3d2d_device."""

    def __init__(self, case):
        self.nkp = [len(k) for k in case["kps"]]
        self.pairs = case["pairs"]
        self.dk = [torch.from_numpy(np.ascontiguousarray(k)).cuda() for k in case["kps"]]
        self.dm = torch.from_numpy(case["matches"].view(np.uint8)).cuda()
        self.do = torch.from_numpy(case["offsets"]).cuda()

    def merge(self, cloud, new, D, F):
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (*cloud, *new)]
        r = scene.merge_pointcloud_3d2d_device([k.data_ptr() for k in self.dk], self.nkp, self.pairs, self.dm.data_ptr(),
                                               self.do.data_ptr(), *t, D, F)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in r.items()}


def run_settings(call, exp, exp_stats=None):
    """`call()` under every setting: each result equals the restatement's, the statistics agree with each other (and
    with the restatement's where given), and the path is the one the setting asks for."""
    stats = []
    for s in SETTINGS:
        scene.merge_set_max_rounds(s)
        assert_equal(call(), exp)
        stats.append(scene.merge_last_stats())
        path = scene.merge_last_path()
        if s == 0:
            assert path["host_fallback"] == 0 and path["rounds"] >= 1, path
        if s == -1:
            assert path["host_fallback"] == 1 and path["rounds"] == 0, path
        if s == 1:
            # one round decides exactly the calls without a link: any link makes a chain of two
            assert path["rounds"] == 1 and path["host_fallback"] == int(stats[-1]["links"] > 0), (path, stats[-1])
    assert stats[0] == stats[1] == stats[2], stats
    if exp_stats is not None:
        assert stats[0]["merged_dynamic"] == exp_stats["dynamic"], (stats, exp_stats)
        assert stats[0]["merged_static"] == exp_stats["merged"] - exp_stats["dynamic"], (stats, exp_stats)
    return stats[0]


# ---- 1. every path gives the same answer -------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers_on_every_path(name):
    a, exp = KNOWN[name]
    st = {}
    assert_equal(merge_ref.merge(*a, stats=st), exp)
    run_settings(lambda: scene.merge_pointcloud_3d2d(*a), exp, st)


@pytest.mark.parametrize("D", merge_cases.D_SWEEP)
def test_scene_on_every_path_host_and_device_inputs(case, D):
    st = {}
    exp = merge_ref.merge(*merge_cases.args(case), D, 20.0, stats=st)
    host = run_settings(lambda: scene.merge_pointcloud_3d2d(*merge_cases.args(case), D, 20.0), exp, st)
    g = DeviceGraph(case)
    dev = run_settings(lambda: g.merge(case["cloud"], case["new"], D, 20.0), exp, st)
    assert host == dev
    print("D", D, "stats", host)


# ---- 2. dependency chains ----------------------------------------------------------------------------------------

DELTA = 0.25


def chain_case(L):
    """Shots 0..L with one keypoint each, pair (i, i + 1) with the single match kp(i, 0) <-> kp(i + 1, 0), an empty
    cloud; element i < L holds the records (i, kp(i, 0)) and (i + 1, kp(i + 1, 0)) and lies at (0, 0, i * DELTA).
    Element i shares the record of shot i with element i - 1, so it is linked to it and can only be decided after it:
    the longest chain of the link DAG is 0 -> 1 -> ... -> L - 1, L elements, whatever the distances decide."""
    graph = merge_cases._graph([(i, i + 1) for i in range(L)], [[(0, 0, 1.0)] for _ in range(L)], n_shots=L + 1, n_kp=1)
    new = merge_cases._cloud([((0.0, 0.0, i * DELTA), [merge_cases._kp(i, 0), merge_cases._kp(i + 1, 0)]) for i in range(L)])
    return (*graph, *merge_cases._cloud([]), *new), L


@pytest.mark.parametrize("L", [1, 2, 3, 63, 64, 65, 257])
def test_chain_takes_as_many_rounds_as_it_is_long(L):
    a, depth = chain_case(L)
    for D in (1.5 * DELTA, 0.0, INF):   # merge and append alternate; every element appended; every element merged
        exp = merge_ref.merge(*a, D, 20.0)
        if D == 1.5 * DELTA:
            assert exp["merge_distance"].tolist() == [-1.0 if i % 2 == 0 else DELTA for i in range(L)]
        scene.merge_set_max_rounds(L + 1)
        assert_equal(scene.merge_pointcloud_3d2d(*a, D, 20.0), exp)
        path = scene.merge_last_path()
        assert path["host_fallback"] == 0 and path["rounds"] == depth, (D, path)


@pytest.mark.parametrize("L,fallback", [(6, 0), (20, 1)])
def test_chain_beyond_the_cap_finishes_on_the_host(L, fallback):
    a, depth = chain_case(L)
    exp = merge_ref.merge(*a, 1.5 * DELTA, 20.0)
    scene.merge_set_max_rounds(8)
    got = scene.merge_pointcloud_3d2d(*a, 1.5 * DELTA, 20.0)
    path = scene.merge_last_path()
    assert path["host_fallback"] == fallback and path["rounds"] == min(depth, 8), path
    assert_equal(got, exp)
    stats = scene.merge_last_stats()
    scene.merge_set_max_rounds(L + 1)
    assert_equal(scene.merge_pointcloud_3d2d(*a, 1.5 * DELTA, 20.0), got)
    assert scene.merge_last_stats() == stats and scene.merge_last_path()["host_fallback"] == 0


# ---- 3. dedupe groups --------------------------------------------------------------------------------------------

def dedupe_case(n, into_appended):
    """One point P holding 3 records and n elements linked to it and within D of it (pair (0, 1) matches P's keypoint
    0 of shot 0 with keypoint j of shot 1, element j's own record).  Element j also carries a record P holds (element
    5 with -0.0 against P's +0.0) and a record shared with its neighbour (2m and 2m + 1: the second finds it accepted
    earlier in the walk); elements 7 and 8 carry the same NaN record, which is always appended.  into_appended: the
    cloud is empty and P is the first new element, so the n elements merge into a point appended in the same call."""
    kp = merge_cases._kp
    graph = merge_cases._graph([(0, 1)], [[(0, j, 1.0) for j in range(n)]], n_shots=4, n_kp=max(n, 1))
    P = ((0.0, 0.0, 0.0), [kp(0, 0), (2, 27.0, 7.0), (3, 0.0, 5.0)])
    new = []
    for j in range(n):
        rec = [kp(1, j), (3, -0.0, 5.0) if j == 5 else (2, 27.0, 7.0), (3, 100.0 + j // 2, 1.0)]
        if j in (7, 8):
            rec.insert(1, (3, float("nan"), 5.0))
        new.append(((0.0, 0.0, 1e-3 * (j % 5)), rec))
    if into_appended:
        return (*graph, *merge_cases._cloud([]), *merge_cases._cloud([P] + new), 0.02, 20.0)
    return (*graph, *merge_cases._cloud([P]), *merge_cases._cloud(new), 0.02, 20.0)


@pytest.mark.parametrize("into_appended", [False, True])
@pytest.mark.parametrize("n", [1, 2, 70])
def test_dedupe_group_walk(n, into_appended):
    a = dedupe_case(n, into_appended)
    exp = merge_ref.merge(*a)
    first = 1 if into_appended else 0
    assert (exp["target"][first:] == 0).all() and len(exp["xyz"]) == 1          # one group of n elements
    assert exp["origin_offsets"][-1] == 3 + n + (n + 1) // 2 + min(max(n - 7, 0), 2)   # own, shared once a pair, NaN records
    scene.merge_set_max_rounds(0)
    assert_equal(scene.merge_pointcloud_3d2d(*a), exp)
    path = scene.merge_last_path()
    assert path["host_fallback"] == 0 and path["rounds"] == (2 if into_appended else 1), path
    scene.merge_set_max_rounds(-1)
    assert_equal(scene.merge_pointcloud_3d2d(*a), exp)


# ---- 4. the cloud does not cross ---------------------------------------------------------------------------------

def padded(cloud, n_pad):
    """n_pad more points behind the cloud: 10 apart and far from every element, each with one record at a position
    that is no keypoint's, so no match names it."""
    xyz, off, shot, xy = cloud
    i = np.arange(n_pad, dtype=np.float64)
    return (np.concatenate([xyz, np.stack([1000.0 + 10.0 * i, 0 * i, 0 * i], 1)]),
            np.concatenate([off, off[-1] + 1 + np.arange(n_pad, dtype=np.int64)]),
            np.concatenate([shot, np.zeros(n_pad, np.int32)]),
            np.concatenate([xy, np.stack([5000.0 + i, 7.0 + 0 * i], 1)]))


@pytest.mark.parametrize("n_pad", [257, SCAN_BLOCK * SCAN_BLOCK])   # the second: beyond one block sum per top-level thread
def test_host_traffic_does_not_depend_on_the_cloud(head, n_pad):
    c, exp0 = head
    g = DeviceGraph(c)
    D, F = merge_cases.D_MID, 20.0
    n_shots, n_pairs = len(c["kps"]), len(c["pairs"])
    assert_equal(g.merge(c["cloud"], c["new"], D, F), exp0)
    base = scene.merge_last_path()
    big = padded(c["cloud"], n_pad)
    assert len(big[0]) > n_pad >= 257
    exp = merge_ref.merge(*merge_cases.args(c, cloud=big), D, F)
    assert_equal(g.merge(big, c["new"], D, F), exp)
    path = scene.merge_last_path()
    print("n_pad", n_pad, "unpadded", base, "padded", path)
    assert path["host_fallback"] == 0 and path == base
    assert path["host_bytes"] <= 4096 + 64 * (n_shots + n_pairs) + 64 * path["rounds"]
    n0 = len(c["cloud"][0])   # the padding takes no part: the same decisions, the appended points n_pad further back
    assert np.array_equal(exp["target"], np.where(exp0["target"] >= n0, exp0["target"] + n_pad, exp0["target"]))
    # the host resolution stages the cloud: its traffic grows with the padding
    scene.merge_set_max_rounds(-1)
    g.merge(c["cloud"], c["new"], D, F)
    staged0 = scene.merge_last_path()["host_bytes"]
    assert_equal(g.merge(big, c["new"], D, F), exp)
    staged = scene.merge_last_path()["host_bytes"]
    assert staged >= staged0 + n_pad * (3 * 8 + 8 + 4 + 2 * 8) and staged0 > path["host_bytes"]


# ---- 5. validation in device mode --------------------------------------------------------------------------------

def _descending(off):
    off = off.copy()
    off[1], off[2] = off[2], off[1] - 1   # ... 4, 1 ...: descends, the last entry stays
    return off


def _with_shot(shot, value):
    shot = shot.copy()
    shot[len(shot) // 2] = value
    return shot


@pytest.mark.parametrize("which", ["cloud", "new"])
@pytest.mark.parametrize("what", ["descending", "shot_negative", "shot_n_shots"])
def test_device_mode_validation(head, which, what):
    c, exp = head
    g = DeviceGraph(c)
    D, F = merge_cases.D_MID, 20.0
    xyz, off, shot, xy = c[which]
    broken = {"descending": (xyz, _descending(off), shot, xy), "shot_negative": (xyz, off, _with_shot(shot, -1), xy),
              "shot_n_shots": (xyz, off, _with_shot(shot, len(c["kps"])), xy)}[what]
    clouds = dict(cloud=c["cloud"], new=c["new"])
    clouds[which] = broken
    message = which + (" origin offsets do not ascend" if what == "descending" else " origin shot out of range")
    with pytest.raises(ValueError, match=message):
        g.merge(clouds["cloud"], clouds["new"], D, F)
    assert_equal(g.merge(c["cloud"], c["new"], D, F), exp)
    if which == "cloud":   # also with nothing new: the cloud is checked before it goes through
        none = merge_cases.slice_new(c["new"], 0, 0)
        with pytest.raises(ValueError, match=message):
            g.merge(broken, none, D, F)
        through = g.merge(c["cloud"], none, D, F)
        assert np.array_equal(through["origin_offsets"], c["cloud"][1])


# ---- 6. end to end -----------------------------------------------------------------------------------------------

def test_reconstruction_is_the_same_with_less_handoff():
    sc = sfm_cases.scene(5, 300, noise=0.3, wrong=0.1, graph="complete", seed=11)
    runs = []
    for s in (0, -1):
        scene.merge_set_max_rounds(s)
        ba.release_cache()
        runs.append(sfm.triangulate(sc["keypoints"], sc["shot_size"], sfm_cases.camera(), ba.CAM_SIMPLE_RADIAL, sc["pairs"],
                                    sc["matches"], sc["offsets"], sc["homography"], sfm.default_params()))
    new, old = runs
    n_arrays = 0
    for k in new:
        if k == "timing":
            continue
        a, b = new[k], old[k]
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
            n_arrays += 1
        elif k == "camera":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), k
        elif k == "summary":   # the counts; step_wall_ms is a clock
            assert {n: v for n, v in a.items() if n != "step_wall_ms"} == {n: v for n, v in b.items() if n != "step_wall_ms"}
        else:
            assert repr(a) == repr(b), k
    assert n_arrays >= 8 and len(new["xyz"]) > 0
    tn, to = new["timing"]["merge"], old["timing"]["merge"]
    print("merge row: device resolution", tn, "host resolution", to)
    assert tn["calls"] == to["calls"] > 0 and 0 < tn["handoff_bytes"] < to["handoff_bytes"]
