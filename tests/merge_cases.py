"""Shared fixed-seed cases for the point-cloud merge (Scene::mergePointcloudElement3d2d, Scene.cpp:470-567).
Inputs only — the expected outputs come from tests/merge_ref.py.

scene_case(): tri_cases' six shots, cameras and landmarks, observed with `noise` px; track-forming match
lists (a landmark matched in A-B is, with probability, also matched in A-N and B-N, through the same
keypoints), DMatch distances spread over [0, 1] with a few negative and NaN ones, one duplicated unordered
pair and one pair of a shot with itself in the pair list.  The cloud is tests/tri_ref.py's triangulation of
the first pair plus copies of some of its points (equal distances: ties); the new elements are the
triangulations of the other pairs, pair-major.

known_cases(): hand-built answers of a handful of points each, name -> (arguments, expected).
"""
import numpy as np

from sfmx.matching import DMATCH_DTYPE
import tri_cases
import tri_ref

N_TRACK = 420            # landmarks the match lists draw from
PAIRS = [(0, 1), (1, 2), (0, 2), (2, 3), (1, 3), (2, 1), (3, 4), (2, 4), (3, 3), (4, 5), (5, 3)]
LENGTHS = [330, 300, 280, 300, 260, 120, 280, 240, 6, 257, 200]
N_DUPLICATED = 40        # cloud points stored twice
D_MID = 0.05             # merges part of the linked elements at 0.7 px noise (asserted in test_merge_ref.py)
D_SWEEP = (0.0, 0.01, D_MID)
F_SWEEP = (20.0, 0.5, -1.0)
INF_SLICE = 60           # D = inf makes every cloud point a candidate: a slice of the elements only


def scene_case(noise=0.7, seed=20261020, clean=False):
    """clean: no wrong partners (every 12th match of a pair otherwise joins keypoints of two different
    landmarks) and an empty list for the self pair (3, 3), whose same-pose triangulations are no landmarks:
    every link then joins two observations of one landmark.
    -> dict(kps, pairs, matches, offsets, cloud = (xyz, offsets, shot, xy), new = (xyz, offsets, shot, xy))."""
    rng = np.random.default_rng(seed)
    poses = tri_cases.arc_poses()
    land = tri_cases.landmarks(rng)
    kps, slot = tri_cases.observe(land, poses, noise, rng)
    lists = []
    for (L, R), m in zip(PAIRS, LENGTHS):
        js = rng.choice(N_TRACK, m, replace=False)
        q, t = slot[L][js], slot[R][js].copy()
        if L != R and not clean:
            t[11::12] = slot[R][rng.integers(0, N_TRACK, len(t[11::12]))]     # wrong partners: links without nearness
        lists.append(np.stack([q, t], axis=1)[:0 if clean and L == R else m])
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    m = np.zeros(int(off[-1]), DMATCH_DTYPE)
    qt = np.concatenate(lists)
    m["queryIdx"], m["trainIdx"] = qt[:, 0], qt[:, 1]
    dist = rng.uniform(0.0, 1.0, len(m)).astype(np.float32)
    dist[5::17] *= -1.0
    dist[3::101] = np.nan
    dist[7::53] = 0.5
    m["distance"] = dist
    pairs = np.array(PAIRS, np.int32)
    tri = tri_ref.triangulate_matches(kps, tri_cases.CAMERAS, tri_cases.SHOT_CAMERA, poses, pairs, m, off)
    k0 = int(tri["point_offsets"][1])
    dup = rng.choice(k0, N_DUPLICATED, replace=False)
    idx = np.concatenate([np.arange(k0), dup])
    rec = (2 * idx[:, None] + np.arange(2)[None, :]).reshape(-1)
    cloud = (tri["xyz"][idx].copy(), 2 * np.arange(len(idx) + 1, dtype=np.int64), tri["origin_shot"][rec].copy(),
             tri["origin_xy"][rec].copy())
    new = (tri["xyz"][k0:].copy(), 2 * np.arange(tri["n_points"] - k0 + 1, dtype=np.int64),
           tri["origin_shot"][2 * k0:].copy(), tri["origin_xy"][2 * k0:].copy())
    return dict(kps=kps, pairs=pairs, matches=m, offsets=off, cloud=cloud, new=new)


def slice_new(new, a, b):
    """Elements a..b of a (xyz, offsets, shot, xy) cloud."""
    xyz, off, shot, xy = new
    return xyz[a:b], off[a:b + 1] - off[a], shot[off[a]:off[b]], xy[off[a]:off[b]]


def args(case, new=None, cloud=None):
    return (case["kps"], case["pairs"], case["matches"], case["offsets"], *(cloud or case["cloud"]), *(new or case["new"]))


def as_cloud(r):
    """A merge result as the cloud of the next call."""
    return r["xyz"], r["origin_offsets"], r["origin_shot"], r["origin_xy"]


# ---- hand-built known answers ------------------------------------------------------------------------

def _graph(pairs, lists, n_shots=4, n_kp=8):
    """Shot s holds keypoints (10 s + k, k) for k < n_kp; lists[p] = [(queryIdx, trainIdx, distance)]."""
    kps = [np.array([[10.0 * s + k, float(k)] for k in range(n_kp)], np.float32) for s in range(n_shots)]
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    m = np.zeros(int(off[-1]), DMATCH_DTYPE)
    flat = [x for lst in lists for x in lst]
    if flat:
        m["queryIdx"], m["trainIdx"], m["distance"] = [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat]
    return kps, np.array(pairs, np.int32).reshape(-1, 2), m, off


def _kp(s, k):
    return (s, 10.0 * s + k, float(k))


def _cloud(points):
    """points: [((x, y, z), [(shot, x, y), ...])] -> (xyz, offsets, shot, xy)."""
    xyz = np.array([p[0] for p in points], np.float64).reshape(-1, 3)
    off = np.zeros(len(points) + 1, np.int64)
    off[1:] = np.cumsum([len(p[1]) for p in points])
    recs = [r for p in points for r in p[1]]
    return (xyz, off, np.array([r[0] for r in recs], np.int32),
            np.array([[r[1], r[2]] for r in recs], np.float64).reshape(-1, 2))


def _expect(points, target, dist):
    xyz, off, shot, xy = _cloud(points)
    return dict(xyz=xyz, origin_offsets=off, origin_shot=shot, origin_xy=xy, target=np.array(target, np.int32),
                merge_distance=np.array(dist, np.float64))


def known_cases():
    """name -> (args tuple for merge(..., D, F), expected dict)."""
    out = {}
    nan = float("nan")
    g01 = _graph([(0, 1)], [[(0, 0, 1.0), (1, 1, 1.0), (2, 2, 1.0)]])
    A, B = ((0, 0, 0), [_kp(0, 0)]), ((5, 0, 0), [_kp(0, 1)])
    E = ((0, 0.006, 0.008), [_kp(1, 0), _kp(2, 7)])                  # distance 0.01 from A (up to rounding)

    def dist(a, b):
        dx, dy, dz = (np.float64(a[i]) - np.float64(b[i]) for i in range(3))
        return float(np.sqrt((dx * dx + dy * dy) + dz * dz))

    # linked and near -> merged (records appended after the old ones)
    out["linked_near"] = ((*g01, *_cloud([A, B]), *_cloud([E]), 0.02, 20.0),
                          _expect([(A[0], A[1] + E[1]), B], [0], [dist(A[0], E[0])]))
    # near but unlinked (no DMatch holds its keypoint)
    E2 = ((0, 0, 0.001), [_kp(1, 5)])
    out["near_unlinked"] = ((*g01, *_cloud([A, B]), *_cloud([E2]), 0.02, 20.0), _expect([A, B, E2], [2], [-1.0]))
    # linked but d > D
    out["linked_far"] = ((*g01, *_cloud([A, B]), *_cloud([E]), 0.005, 20.0), _expect([A, B, E], [2], [-1.0]))
    # |distance| > F -> appended; == F -> merged (negative distance: abs)
    gF = _graph([(0, 1)], [[(0, 0, -0.75), (1, 1, 0.5)]])
    E3 = ((5, 0, 0.001), [_kp(1, 1)])
    out["feature_distance_above"] = ((*gF, *_cloud([A, B]), *_cloud([E]), 0.02, 0.5), _expect([A, B, E], [2], [-1.0]))
    out["feature_distance_equal"] = ((*gF, *_cloud([A, B]), *_cloud([E, E3]), 0.02, 0.75),
                                     _expect([(A[0], A[1] + E[1]), (B[0], B[1] + E3[1])], [0, 1],
                                             [dist(A[0], E[0]), dist(B[0], E3[0])]))
    # a distance tie -> lower index; a strictly nearer later point wins over an earlier one
    A2, A3 = ((0, 0, 0), [_kp(0, 0)]), ((0, 0.006, 0.007), [_kp(0, 0)])
    out["tie_lower_index"] = ((*g01, *_cloud([B, A, A2]), *_cloud([E]), 0.02, 20.0),
                              _expect([B, (A[0], A[1] + E[1]), A2], [1], [dist(A[0], E[0])]))
    out["nearer_later_wins"] = ((*g01, *_cloud([A, A3]), *_cloud([E]), 0.02, 20.0),
                                _expect([A, (A3[0], A3[1] + E[1])], [1], [dist(A3[0], E[0])]))
    # qualifies only through a record merged earlier in the same call: E links A (0-1), E4 links E's shot-2
    # record through pair (2, 3) and nothing of A
    g3 = _graph([(0, 1), (2, 3)], [[(0, 0, 1.0)], [(7, 4, 1.0)]])
    E4 = ((0, 0.001, 0), [_kp(3, 4)])
    out["through_same_call_record"] = ((*g3, *_cloud([A, B]), *_cloud([E, E4]), 0.02, 20.0),
                                       _expect([(A[0], A[1] + E[1] + E4[1]), B], [0, 0], [dist(A[0], E[0]), dist(A[0], E4[0])]))
    # merges into an element appended earlier in the same call
    out["into_appended"] = ((*g3, *_cloud([B]), *_cloud([E, E4]), 0.02, 20.0),
                            _expect([B, (E[0], E[1] + E4[1])], [1, 1], [-1.0, dist(E[0], E4[0])]))
    # the lowest static qualifier N is NaN, a lower-index point P qualifies only through the record Ea brought in
    # the same call (finite, so the fold goes on) and the nearest qualifier S is static: a static merge
    gc = _graph([(0, 1), (2, 3)], [[(0, 0, 1.0), (3, 3, 1.0)], [(7, 4, 1.0)]])
    P, Nn, S = ((0, 0, 0.005), [_kp(0, 3)]), ((nan, 0, 0), [_kp(0, 0)]), ((0, 0, 0), [_kp(0, 0)])
    Ea, Eb = ((0, 0, 0.005), [_kp(1, 3), _kp(2, 7)]), ((0, 0, 0.001), [_kp(1, 0), _kp(3, 4)])
    out["nan_static_first_behind_dynamic"] = ((*gc, *_cloud([P, Nn, S]), *_cloud([Ea, Eb]), 0.02, 20.0),
                                              _expect([(P[0], P[1] + Ea[1]), Nn, (S[0], S[1] + Eb[1])], [0, 2],
                                                      [0.0, dist(S[0], Eb[0])]))
    # NaN coordinates: near everything; wins only as the lowest-index qualifier
    N = ((nan, 0, 0), [_kp(0, 0)])
    out["nan_point_first_wins"] = ((*g01, *_cloud([N, A]), *_cloud([E]), 0.02, 20.0),
                                   _expect([(N[0], N[1] + E[1]), A], [0], [nan]))
    out["nan_point_later_loses"] = ((*g01, *_cloud([A, N]), *_cloud([E]), 0.02, 20.0),
                                    _expect([(A[0], A[1] + E[1]), N], [0], [dist(A[0], E[0])]))
    En = ((nan, nan, nan), [_kp(1, 0)])
    out["nan_element"] = ((*g01, *_cloud([B, A, A2]), *_cloud([En]), 0.0, 20.0),
                          _expect([B, (A[0], A[1] + En[1]), A2], [1], [nan]))
    # a record already held is not added twice (also -0 == +0), a NaN record always is
    H = ((0, 0, 0), [_kp(0, 0), (2, 27.0, 7.0), (3, 0.0, 5.0)])
    E5 = ((0, 0, 0), [_kp(1, 0), (2, 27.0, 7.0), (3, -0.0, 5.0), (3, nan, 5.0), _kp(1, 0), (3, nan, 5.0)])
    out["dedupe_and_nan_record"] = ((*g01, *_cloud([H]), *_cloud([E5]), 0.02, 20.0),
                                    _expect([(H[0], H[1] + [_kp(1, 0), (3, nan, 5.0), (3, nan, 5.0)])], [0], [0.0]))
    # a duplicated unordered pair: only the first is used (the second alone would link E to A)
    gd = _graph([(1, 0), (0, 1)], [[(5, 5, 1.0)], [(0, 0, 1.0)]])
    out["duplicate_pair_second_ignored"] = ((*gd, *_cloud([A, B]), *_cloud([E]), 0.02, 20.0), _expect([A, B, E], [2], [-1.0]))
    gd2 = _graph([(1, 0), (0, 1)], [[(0, 0, 1.0)], [(5, 5, 1.0)]])
    out["duplicate_pair_first_reversed"] = ((*gd2, *_cloud([A, B]), *_cloud([E]), 0.02, 20.0),
                                            _expect([(A[0], A[1] + E[1]), B], [0], [dist(A[0], E[0])]))
    # a record not representable as float never links (keypoint 0.1f as double is not 0.1)
    gr = _graph([(0, 1)], [[(0, 0, 1.0)]])
    gr[0][0][0] = (0.1, 0.0)
    Ar = ((0, 0, 0), [(0, 0.1, 0.0)])
    Af = ((0, 0, 0), [(0, float(np.float32(0.1)), 0.0)])
    out["unrepresentable_record"] = ((*gr, *_cloud([Ar]), *_cloud([E]), 0.02, 20.0), _expect([Ar, E], [1], [-1.0]))
    out["representable_record"] = ((*gr, *_cloud([Af]), *_cloud([E]), 0.02, 20.0),
                                   _expect([(Af[0], Af[1] + E[1])], [0], [dist(Af[0], E[0])]))
    # out-of-range match indices and a pair of a shot with itself never link
    go = _graph([(0, 0), (0, 1)], [[(0, 0, 1.0)], [(0, 8, 1.0), (-1, 0, 1.0)]])
    out["bad_indices_and_self_pair"] = ((*go, *_cloud([A, B]), *_cloud([E, ((0, 0, 0), [_kp(0, 0)])]), 0.02, 20.0),
                                        _expect([A, B, E, ((0, 0, 0), [_kp(0, 0)])], [2, 3], [-1.0, -1.0]))
    # thresholds: D < 0 keeps only NaN distances, D = inf takes any linked point, F < 0 links nothing
    E0 = ((0, 0, 0), [_kp(1, 0)])
    out["negative_D"] = ((*g01, *_cloud([A, N]), *_cloud([E0]), -1.0, 20.0), _expect([A, (N[0], N[1] + E0[1])], [1], [nan]))
    E6 = ((1e9, 0, 0), [_kp(1, 1)])
    out["infinite_D"] = ((*g01, *_cloud([A, B]), *_cloud([E6]), float("inf"), 20.0),
                         _expect([A, (B[0], B[1] + E6[1])], [1], [dist(B[0], E6[0])]))
    out["negative_F"] = ((*g01, *_cloud([A, B]), *_cloud([E0]), 0.02, -1.0), _expect([A, B, E0], [2], [-1.0]))
    # empty cloud, an element without records, an empty point in the cloud
    Z = ((1, 1, 1), [])
    E7 = ((0, 0, 0.001), [_kp(0, 0)])
    out["empty_cloud_and_recordless"] = ((*g01, *_cloud([]), *_cloud([Z, E0, E7]), 0.02, 20.0),
                                         _expect([Z, (E0[0], E0[1] + E7[1])], [0, 1, 1], [-1.0, -1.0, dist(E0[0], E7[0])]))
    out["empty_point_in_cloud"] = ((*g01, *_cloud([Z, A, Z]), *_cloud([E]), 0.02, 20.0),
                                   _expect([Z, (A[0], A[1] + E[1]), Z], [1], [dist(A[0], E[0])]))
    return out
