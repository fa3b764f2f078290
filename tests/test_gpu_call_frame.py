"""GPU: the life of a per-device slot across calls (csrc/device_call.hpp), for nine entry points that use it:
homography ratios, triangulation, relative pose, registration pose, distinct 3D-2D points, cloud neighbour distances,
the 3D-2D search and its count (one slot for both), the cloud merge (a slot for the call and one for its link list).

The parity tests of each module check one call against its restatement.  Here one process makes small and large
calls in turn on the same slot, with host and with device arrays: the device block regrows for the large call
(four copies of the small one's pairs or sets, more than 1.25 x its need, wherever no earlier test of the process
has grown that slot further), is reused by the next small one, and its host-staging parts come and go.  Every pair
and set seeds its own RNG, so the large call's outputs are the small call's repeated; the cloud, where copies would
be duplicates, uses the golden cloud and one of four times as many points against tests/cloud_ref.py; the 3D-2D
search, its count and the merge use a small and a large case of their own suites against the oracle and
tests/merge_ref.py.  A call that is refused after its slot was opened (a match index past its image's keypoints:
found by the kernels with device inputs, on the host with host inputs for the 3D-2D search and its count; for the
merge, offsets read back from the device that do not start at 0) leaves the slot usable.
Everything is compared as bytes, so NaN outputs count."""
import numpy as np
import pytest
import torch

from sfmx import cloud, homography, pnp, pose, scene, triangulate
from sfmx.matching import DMATCH_DTYPE
import cloud_cases
import cloud_ref
import fixtures
import homog_cases
import merge_cases
import merge_ref
import pnp_cases
import pnp_ref
import pose_cases
import scene_cases
import tri_cases

pytestmark = pytest.mark.gpu

REPS = 4


def tile_offsets(off, reps):
    off = np.asarray(off, np.int64)
    return np.concatenate([off[:-1] + r * off[-1] for r in range(reps)] + [[reps * off[-1]]]).astype(np.int64)


def tile_rows(a, reps):
    return np.tile(a, (reps,) + (1,) * (np.ndim(a) - 1))


def to_numpy(d):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def assert_same(got, exp, what):
    assert set(got) == set(exp), (what, sorted(got), sorted(exp))
    for k in exp:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, e.shape, g.dtype, e.dtype)
        assert g.tobytes() == e.tobytes(), (what, k)


class Homography:
    def __init__(self):
        self.kps, self.sizes, self.pairs, self.m, self.off = homog_cases.edge_case()

    def run(self, reps, dev, m=None):
        pairs, m, off = tile_rows(self.pairs, reps), np.tile(self.m, reps), tile_offsets(self.off, reps)
        if not dev:
            return {"ratio": homography.homography_ratios(self.kps, self.sizes, pairs, m, off)}
        dk = [torch.from_numpy(k).cuda() for k in self.kps]
        dm, do = torch.from_numpy(m.view(np.uint8)).cuda(), torch.from_numpy(off).cuda()
        return {"ratio": homography.homography_ratios_device([t.data_ptr() for t in dk], [len(k) for k in self.kps], self.sizes,
                                                             pairs, dm.data_ptr(), do.data_ptr())}

    def tiled(self, a, reps):
        return {"ratio": np.tile(a["ratio"], reps)}


class Triangulate:
    KEYS = ("point_offsets", "xyz", "match", "origin_offsets", "origin_shot", "origin_xy", "err")

    def __init__(self):
        self.c = tri_cases.small_case()

    def run(self, reps, dev, m=None):
        kps, cams, sc, poses, pairs, m0, off = tri_cases.args(self.c)
        m = np.tile(m0 if m is None else m, reps)
        pairs, off = tile_rows(pairs, reps), tile_offsets(off, reps)
        if not dev:
            r = triangulate.triangulate_matches(kps, cams, sc, poses, pairs, m, off)
        else:
            dk = [torch.from_numpy(k).cuda() for k in kps]
            dm, do = torch.from_numpy(m.view(np.uint8)).cuda(), torch.from_numpy(off).cuda()
            r = to_numpy(triangulate.triangulate_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, poses,
                                                                pairs, dm.data_ptr(), do.data_ptr(), len(m), with_err=True))
        out = {k: r[k] for k in self.KEYS}
        out["n_points"] = np.int64(r["n_points"])
        return out

    def tiled(self, a, reps):
        k, n = int(a["n_points"]), len(self.c["matches"])
        return dict(n_points=np.int64(reps * k), point_offsets=tile_offsets(a["point_offsets"], reps), xyz=tile_rows(a["xyz"], reps),
                    match=(a["match"][None, :] + n * np.arange(reps)[:, None]).reshape(-1),
                    origin_offsets=2 * np.arange(reps * k + 1, dtype=np.int64), origin_shot=np.tile(a["origin_shot"], reps),
                    origin_xy=tile_rows(a["origin_xy"], reps), err=tile_rows(a["err"], reps))

    def bad_matches(self):
        bad = self.c["matches"].copy()
        bad["trainIdx"][1500] = 10 ** 6
        return bad


class Pose:
    KEYS = ("status", "E", "pose", "mask", "n_ransac_inliers", "n_inliers", "matches", "pair_offsets")

    def __init__(self):
        self.c = pose_cases.small_case()

    def run(self, reps, dev, m=None):
        kps, cams, sc, size, pairs, m0, off = pose_cases.args(self.c)
        m = np.tile(m0 if m is None else m, reps)
        pairs, off = tile_rows(pairs, reps), tile_offsets(off, reps)
        if not dev:
            r = pose.relative_poses(kps, cams, sc, size, pairs, m, off, threshold=-1.0)
        else:
            dk = [torch.from_numpy(k).cuda() for k in kps]
            dm, do = torch.from_numpy(m.view(np.uint8)).cuda(), torch.from_numpy(off).cuda()
            r = to_numpy(pose.relative_poses_device([t.data_ptr() for t in dk], [len(k) for k in kps], cams, sc, size, pairs,
                                                    dm.data_ptr(), do.data_ptr(), len(m), threshold=-1.0))
            r["matches"] = r["matches"][:int(r["pair_offsets"][-1])].reshape(-1).view(DMATCH_DTYPE)
        return {k: r[k] for k in self.KEYS}

    def tiled(self, a, reps):
        out = {k: tile_rows(a[k], reps) for k in self.KEYS if k != "pair_offsets"}
        out["pair_offsets"] = tile_offsets(a["pair_offsets"], reps)
        return out

    def bad_matches(self):
        p = self.c["names"].index("len64")
        bad = self.c["matches"].copy()
        bad["trainIdx"][self.c["offsets"][p] + 9] = len(self.c["kps"][self.c["pairs"][p][1]])
        return bad


class Register:
    KEYS = ("status", "pose", "ransac_pose", "mask", "n_inliers", "inlier_ratio", "refit_start")

    def __init__(self):
        self.c = pnp_cases.small_case()

    def run(self, reps, dev, m=None):
        p3, p2, off, ss, cams, sc, size = pnp_cases.args(self.c)
        p3, p2, off, ss = tile_rows(p3, reps), tile_rows(p2, reps), tile_offsets(off, reps), np.tile(ss, reps)
        if not dev:
            r = pnp.register_poses(p3, p2, off, ss, cams, sc, size, threshold=-8.0)
        else:
            d3, d2, do = torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda(), torch.from_numpy(off).cuda()
            r = to_numpy(pnp.register_poses_device(d3.data_ptr(), d2.data_ptr(), do.data_ptr(), len(p3), ss, cams, sc, size,
                                                   threshold=-8.0))
        return {k: r[k] for k in self.KEYS}

    def tiled(self, a, reps):
        return {k: tile_rows(a[k], reps) for k in self.KEYS}


class Distinct:
    """300 cloud points with 1 .. 3 origin records each; a third of the records found no keypoint, the others draw
    from 40 image points, so equal (point, image point) records occur.  Copy r of the cloud is moved by 100 r, so
    its records are distinct from every other copy's and the large call's output is the small one's per copy."""

    def __init__(self):
        rng = np.random.default_rng(31)
        n = 300
        self.xyz = rng.uniform(-3, 3, (n, 3))
        self.xyz[7] = self.xyz[2]                      # equal coordinates at different point indices
        self.oo = np.concatenate([[0], np.cumsum(rng.integers(1, 4, n))]).astype(np.int64)
        nr = int(self.oo[-1])
        pool = rng.uniform(0, 640, (40, 2)).astype(np.float32)
        pick = rng.integers(0, 40, nr)
        self.fk = np.where(rng.random(nr) < 1 / 3, -1, pick).astype(np.int32)
        self.fxy = pool[pick]

    def restatement(self):
        e3, e2 = pnp_ref.distinct_3d2d(self.xyz, self.oo, self.fk, self.fxy)
        assert 0 < len(e3) < int((self.fk >= 0).sum())            # something was dropped
        return {"xyz": e3, "xy": e2}

    def run(self, reps, dev, m=None):
        xyz = np.concatenate([self.xyz + 100.0 * r for r in range(reps)])
        oo, fk, fxy = tile_offsets(self.oo, reps), np.tile(self.fk, reps), tile_rows(self.fxy, reps)
        if not dev:
            g3, g2 = pnp.distinct_3d2d_points(xyz, oo, fk, fxy)
        else:
            t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (xyz, oo, fk, fxy)]
            d3, d2 = pnp.distinct_3d2d_points_device(t[0].data_ptr(), len(xyz), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                                     len(fk))
            torch.cuda.synchronize()
            g3, g2 = d3.cpu().numpy(), d2.cpu().numpy()
        return {"xyz": g3, "xy": g2}

    def tiled(self, a, reps):
        return {"xyz": np.concatenate([a["xyz"] + 100.0 * r for r in range(reps)]), "xy": tile_rows(a["xy"], reps)}


class Cloud:
    def __init__(self):
        g = fixtures.load("cloud_small")
        self.x = {1: g["xyz"], REPS: cloud_cases.small_mesh(seed=8, n=REPS * len(g["xyz"]))[0]}
        self.ref = {r: dict(zip(("distance", "neighbor"), cloud_ref.neighbor_distances(x))) for r, x in self.x.items()}
        assert self.ref[1]["distance"].tobytes() == g["distance"].tobytes()

    def run(self, reps, dev, m=None):
        x = self.x[reps]
        d, nb = cloud.neighbor_distances(torch.from_numpy(x).cuda() if dev else x, 0, neighbors=True)
        return to_numpy({"distance": d, "neighbor": nb})

    def restatement(self):
        return self.ref[1]

    def tiled(self, a, reps):
        return self.ref[reps]


class Scene3d2d:
    """The 3D-2D search for one shot and its count for every shot, which share one slot: the small case is
    scene_cases.edge_case(), the large one scene_cases.scene_case(6, 1200, seed=5), both against the oracle's
    find_3d2d_matches.  The search's block, from the part sizes of csrc/scene.hip (every part rounded up to 256
    bytes): small 2 048 bytes with device inputs (six tables, two hash tables of 32 slots) and 4 352 with host inputs;
    large 10 752 (three pairs with shot 2 hold matches, 768 slots of 12 bytes) and 133 888.  The count's tables serve
    every shot and are larger still."""
    SHOT = {1: 0, REPS: 2}

    _SHARED = None   # the cases and the oracle's answers, computed once for both entry points

    def __init__(self):
        if Scene3d2d._SHARED is None:
            Scene3d2d._SHARED = self.cases_and_answers()
        self.case, self.found, self.counts = Scene3d2d._SHARED

    def cases_and_answers(self):
        from oracle import oracle
        self.case = {1: scene_cases.edge_case(), REPS: scene_cases.scene_case(6, 1200, seed=5)}
        self.found, self.counts = {}, {}
        for r, c in self.case.items():
            per_shot = [oracle.find_3d2d_matches(*c, s) for s in range(len(c[0]))]
            k, p = per_shot[self.SHOT[r]]
            xy = np.full((len(k), 2), np.nan, np.float32)
            xy[k >= 0] = c[0][self.SHOT[r]][k[k >= 0]]
            self.found[r] = dict(keypoint=k.astype(np.int32), pair=p.astype(np.int32), xy=xy)
            self.counts[r] = {"count": np.array([(k >= 0).sum() for k, _ in per_shot], np.int32)}
        assert (self.found[1]["keypoint"] >= 0).sum() == 4 and (self.found[REPS]["keypoint"] >= 0).sum() > 100
        return self.case, self.found, self.counts

    def restatement(self):
        return self.expected(1)

    def tiled(self, a, reps):
        return self.expected(reps)

    def device_arrays(self, reps, m):
        kps, pairs, m0, off, oo, osh, oxy = self.case[reps]
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return [d(k) for k in kps], [d(a) for a in ((m0 if m is None else m).view(np.uint8), off, oo, osh, oxy)]

    def bad_matches(self):
        """Host inputs: the index is found on the host, after the slot was opened (device inputs are not read there)."""
        bad = self.case[1][2].copy()
        bad["trainIdx"][1] = len(self.case[1][0][1])   # pair 0 (0, 1): read for shot 0 and by the count
        return bad

    REFUSED_ON_DEVICE = False


class Find3d2d(Scene3d2d):
    def expected(self, reps):
        return self.found[reps]

    def run(self, reps, dev, m=None):
        kps, pairs, m0, off, oo, osh, oxy = self.case[reps]
        shot = self.SHOT[reps]
        if not dev:
            k, p, xy = scene.find_3d2d_matches(kps, pairs, m0 if m is None else m, off, oo, osh, oxy, shot)
            return dict(keypoint=k, pair=p, xy=xy)
        dk, (dm, doff, doo, dsh, dxy) = self.device_arrays(reps, m)
        n = len(osh)
        out = dict(keypoint=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                   pair=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                   xy=torch.zeros((n, 2), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        scene.find_3d2d_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], pairs, dm.data_ptr(), doff.data_ptr(),
                                       doo.data_ptr(), len(oo) - 1, dsh.data_ptr(), dxy.data_ptr(), shot,
                                       out["keypoint"].data_ptr(), out["pair"].data_ptr(), out["xy"].data_ptr())
        return to_numpy(out)


class Count3d2d(Scene3d2d):
    def expected(self, reps):
        return self.counts[reps]

    def run(self, reps, dev, m=None):
        kps, pairs, m0, off, oo, osh, oxy = self.case[reps]
        cand = list(range(len(kps)))
        if not dev:
            return {"count": scene.count_3d2d_matches(kps, pairs, m0 if m is None else m, off, oo, osh, oxy, cand)}
        dk, (dm, doff, doo, dsh, dxy) = self.device_arrays(reps, m)
        out = torch.full((len(cand),), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        scene.count_3d2d_matches_device([t.data_ptr() for t in dk], [len(k) for k in kps], pairs, dm.data_ptr(), doff.data_ptr(),
                                        doo.data_ptr(), len(oo) - 1, dsh.data_ptr(), dxy.data_ptr(), cand, out.data_ptr())
        return to_numpy({"count": out})


class Merge:
    """The small case is the known answer `linked_near` (one new element: no links among new elements, so the call
    makes no use of the link-list slot), the large one merge_cases.scene_case() against tests/merge_ref.py, whose
    dynamic merges are merges through a link between two new elements: that call grows the link-list slot."""
    KEYS = ("xyz", "origin_offsets", "origin_shot", "origin_xy", "target", "merge_distance")

    def __init__(self):
        small, known = merge_cases.known_cases()["linked_near"]
        c = merge_cases.scene_case()
        self.args = {1: small, REPS: (*merge_cases.args(c), merge_cases.D_MID, 20.0)}
        stats = {1: {}, REPS: {}}
        self.ref = {r: merge_ref.merge(*a, stats=stats[r]) for r, a in self.args.items()}
        assert_same(self.ref[1], known, "merge: the known answer")
        assert len(small[8]) == 1 and stats[1]["dynamic"] == 0 and stats[REPS]["dynamic"] > 0

    def restatement(self):
        return self.ref[1]

    def tiled(self, a, reps):
        return self.ref[reps]

    def run(self, reps, dev, m=None, new_offsets=None):
        kps, pairs, m, off, cx, co, cs, cxy, nx, no, ns, nxy, D, F = self.args[reps]
        if not dev:
            r = scene.merge_pointcloud_3d2d(kps, pairs, m, off, cx, co, cs, cxy, nx, no, ns, nxy, D, F)
        else:
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            dk, dm, do = [d(k) for k in kps], d(m.view(np.uint8)), d(off)
            clouds = [d(a) for a in (cx, co, cs, cxy, nx, no if new_offsets is None else new_offsets, ns, nxy)]
            r = to_numpy(scene.merge_pointcloud_3d2d_device([t.data_ptr() for t in dk], [len(k) for k in kps], pairs, dm.data_ptr(),
                                                            do.data_ptr(), *clouds, D, F))
        links = scene.merge_last_stats()["links"]
        assert (links > 0) == (reps == REPS), (reps, links)
        return {k: r[k] for k in self.KEYS}

    REFUSED = "new origin offsets"

    def refused_call(self):
        """Device inputs: the offsets are read back and refused after the slot was opened."""
        self.run(1, True, new_offsets=np.array([1, 2], np.int64))


ENTRIES = {"homography": Homography, "triangulate": Triangulate, "pose": Pose, "register": Register, "distinct": Distinct,
           "cloud": Cloud, "find_3d2d": Find3d2d, "count_3d2d": Count3d2d, "merge": Merge}
_CACHE = {}


def entry(name):
    """The entry point's case and its first small host call (a), made once and left unchanged."""
    if name not in _CACHE:
        e = ENTRIES[name]()
        first = e.run(1, False)
        for v in first.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        if hasattr(e, "restatement"):
            assert_same(first, e.restatement(), name + ": restatement")
        _CACHE[name] = (e, first)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_small_large_small(name, dev):
    e, first = entry(name)
    assert_same(e.run(1, dev), first, "small")
    assert_same(e.run(REPS, dev), e.tiled(first, REPS), "large")
    assert_same(e.run(1, dev), first, "small after large")


@pytest.mark.parametrize("name", list(ENTRIES))
def test_host_and_device_calls_alternate_on_one_slot(name):
    e, first = entry(name)
    large = e.tiled(first, REPS)
    assert_same(e.run(1, False), first, "host small")
    assert_same(e.run(REPS, True), large, "device large")
    assert_same(e.run(1, True), first, "device small")
    assert_same(e.run(REPS, False), large, "host large")
    assert_same(e.run(1, True), first, "device small again")
    assert_same(e.run(1, False), first, "host small again")


@pytest.mark.parametrize("name", ["triangulate", "pose", "find_3d2d", "count_3d2d", "merge"])
def test_call_refused_by_the_kernels_leaves_the_slot_usable(name):
    e, first = entry(name)
    with pytest.raises(ValueError, match=getattr(e, "REFUSED", "keypoints")):
        if hasattr(e, "refused_call"):
            e.refused_call()
        else:
            e.run(1, getattr(e, "REFUSED_ON_DEVICE", True), e.bad_matches())
    assert_same(e.run(1, True), first, "device call after the refused one")
    assert_same(e.run(1, False), first, "host call after the refused one")


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_find_and_count_take_turns_on_their_slot(dev):
    """sfmx_find_3d2d_matches and sfmx_count_3d2d_matches lay their blocks out differently in the same slot."""
    f, f_small = entry("find_3d2d")
    c, c_small = entry("count_3d2d")
    assert_same(f.run(1, dev), f_small, "find small")
    assert_same(c.run(REPS, dev), c.expected(REPS), "count large")
    assert_same(f.run(1, not dev), f_small, "find small after count large")
    assert_same(f.run(REPS, dev), f.expected(REPS), "find large")
    assert_same(c.run(1, dev), c_small, "count small after find large")
    assert_same(c.run(REPS, not dev), c.expected(REPS), "count large again")
    assert_same(f.run(1, dev), f_small, "find small again")
