"""GPU: the life of a per-device slot across calls (csrc/device_call.hpp), for the six entry points that use it:
homography ratios, triangulation, relative pose, registration pose, distinct 3D-2D points, cloud neighbour distances.

The parity tests of each module check one call against its restatement.  Here one process makes small and large
calls in turn on the same slot, with host and with device arrays: the device block regrows for the large call
(four copies of the small one's pairs or sets, more than 1.25 x its need, wherever no earlier test of the process
has grown that slot further), is reused by the next small one, and its host-staging parts come and go.  Every pair
and set seeds its own RNG, so the large call's outputs are the small call's repeated; the cloud, where copies would
be duplicates, uses the golden cloud and one of four times as many points against tests/cloud_ref.py.  A call that
the kernels refuse (a match index past its image's keypoints, device inputs) leaves the slot usable.
Everything is compared as bytes, so NaN outputs count."""
import numpy as np
import pytest
import torch

from sfmx import cloud, homography, pnp, pose, triangulate
from sfmx.matching import DMATCH_DTYPE
import cloud_cases
import cloud_ref
import fixtures
import homog_cases
import pnp_cases
import pnp_ref
import pose_cases
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


ENTRIES = {"homography": Homography, "triangulate": Triangulate, "pose": Pose, "register": Register, "distinct": Distinct,
           "cloud": Cloud}
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


@pytest.mark.parametrize("name", ["triangulate", "pose"])
def test_call_refused_by_the_kernels_leaves_the_slot_usable(name):
    e, first = entry(name)
    with pytest.raises(ValueError, match="keypoints"):
        e.run(1, True, e.bad_matches())
    assert_same(e.run(1, True), first, "device call after the refused one")
    assert_same(e.run(1, False), first, "host call after the refused one")
