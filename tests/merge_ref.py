"""Restatement of the point-cloud merge loop (SfM.cpp:354-363 calling Scene::mergePointcloudElement3d2d,
common/Scene.cpp:470-567) on the origin CSR of include/sfmx_scene.h.

It follows the reference's loops literally: per new element a scan of the whole current cloud with the
near test (:481-488), per candidate every (element record x candidate record) (:498-499), the first pair
in list order joining the two shots (:505-520), a scan of that pair's DMatch list (:524-545), the fold
`best == -1 || best > d` in cloud index order (the reference's single-thread order) and the merge or the
append (:552-567).  numpy vectorises the innermost scans only (the distance over the cloud, the pair list,
one DMatch list); there is no table and no join, so it shares nothing with csrc/merge.hip.

Deviation shared with the library: the CSR carries origin points, so addOrigin's duplicate
test (:205-214) is the record-level one: a record is not added to a point that holds an equal (shot, xy).
A NaN distance is reported as the canonical quiet NaN.
"""
import numpy as np

F64 = np.float64


def point_distance(cloud_xyz, e):
    """cv::norm(candidate - element) for every cloud point: sqrt((dx*dx + dy*dy) + dz*dz) in double."""
    with np.errstate(all="ignore"):
        dx, dy, dz = cloud_xyz[:, 0] - e[0], cloud_xyz[:, 1] - e[1], cloud_xyz[:, 2] - e[2]
        d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    d[np.isnan(d)] = np.nan
    return d


class _Graph:
    def __init__(self, keypoints, pairs, matches, offsets, F):
        self.kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
        self.pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        self.m, self.off, self.F = matches, np.asarray(offsets, np.int64), F64(F)
        self._lists = {}

    def first_pair(self, a, b):
        """Scene.cpp:505-520: the first pair (left, right) == (a, b) or (b, a); -> (pair, a_is_left) or None."""
        L, R = self.pairs[:, 0], self.pairs[:, 1]
        hit = np.flatnonzero(((L == a) & (R == b)) | ((L == b) & (R == a)))
        if not len(hit):
            return None
        p = int(hit[0])
        return p, bool(self.pairs[p, 0] == a and self.pairs[p, 1] == b)

    def pair_list(self, p):
        """The pair's DMatch list as cv::Point2d positions: (left n x 2, right n x 2, admissible n)."""
        if p not in self._lists:
            lst = self.m[self.off[p]:self.off[p + 1]]
            kl, kr = self.kps[self.pairs[p, 0]], self.kps[self.pairs[p, 1]]
            q, t = lst["queryIdx"].astype(np.int64), lst["trainIdx"].astype(np.int64)
            ok = (q >= 0) & (q < len(kl)) & (t >= 0) & (t < len(kr))
            left, right = np.full((len(lst), 2), np.nan), np.full((len(lst), 2), np.nan)
            left[ok], right[ok] = kl[q[ok]].astype(F64), kr[t[ok]].astype(F64)
            with np.errstate(invalid="ignore"):
                ok &= np.abs(lst["distance"]).astype(F64) <= self.F          # abs(float) promoted to double; NaN fails
            self._lists[p] = (left, right, ok)
        return self._lists[p]

    def linked(self, se, qe, sc, qc):
        """Scene.cpp:501-545 for one (element record, candidate record)."""
        if se == sc:
            return False
        fp = self.first_pair(se, sc)
        if fp is None:
            return False
        p, e_is_left = fp
        left, right, ok = self.pair_list(p)
        lp, rp = (qe, qc) if e_is_left else (qc, qe)
        return bool((ok & (left[:, 0] == lp[0]) & (left[:, 1] == lp[1]) & (right[:, 0] == rp[0]) & (right[:, 1] == rp[1])).any())


def merge(keypoints, pairs, matches, offsets, cloud_xyz, cloud_origin_offsets, cloud_origin_shot, cloud_origin_xy,
          new_xyz, new_origin_offsets, new_origin_shot, new_origin_xy, point_merge_distance=0.01,
          feature_merge_distance=20.0, stats=None):
    """-> dict(xyz, origin_offsets, origin_shot, origin_xy, target, merge_distance), as sfmx.merge_pointcloud_3d2d.
    stats (a dict, optional) receives `merged` (elements merged), `dynamic` (merges whose winner qualified
    only through a record added in this call, or is a point appended in this call) and `ties` (merges where
    another qualifying candidate had the winner's distance)."""
    g = _Graph(keypoints, pairs, matches, offsets, feature_merge_distance)
    D = F64(point_merge_distance)
    cx = np.asarray(cloud_xyz, F64).reshape(-1, 3)
    nx = np.asarray(new_xyz, F64).reshape(-1, 3)
    co, no = np.asarray(cloud_origin_offsets, np.int64), np.asarray(new_origin_offsets, np.int64)
    cs, ns = np.asarray(cloud_origin_shot, np.int64), np.asarray(new_origin_shot, np.int64)
    cxy, nxy = np.asarray(cloud_origin_xy, F64).reshape(-1, 2), np.asarray(new_origin_xy, F64).reshape(-1, 2)
    n_cloud, n_new = len(cx), len(nx)
    xyz = np.zeros((n_cloud + n_new, 3))
    xyz[:n_cloud] = cx
    n = n_cloud
    records = [[(int(cs[r]), cxy[r, 0], cxy[r, 1]) for r in range(co[c], co[c + 1])] for c in range(n_cloud)]
    n_initial = [len(r) for r in records]
    target, dist = np.zeros(n_new, np.int32), np.zeros(n_new)
    n_dynamic = n_ties = n_qual = 0
    for e in range(n_new):
        erec = [(int(ns[r]), nxy[r, 0], nxy[r, 1]) for r in range(no[e], no[e + 1])]
        d = point_distance(xyz[:n], nx[e])
        with np.errstate(invalid="ignore"):
            cand = np.flatnonzero(~(d > D))                       # Scene.cpp:483: `if (d > D) continue`
        best, best_c, qualifying = F64(-1.0), -1, []
        for c in cand:
            c = int(c)
            hit = [k for k, (sc, xc, yc) in enumerate(records[c])
                   if any(g.linked(se, (xe, ye), sc, (xc, yc)) for se, xe, ye in erec)]
            if not hit:
                continue
            qualifying.append((c, d[c], min(hit) >= n_initial[c] or c >= n_cloud))
            if best == -1 or best > d[c]:                          # Scene.cpp:533
                best, best_c = d[c], c
        if best_c < 0:
            xyz[n] = nx[e]
            records.append(list(erec))
            n_initial.append(len(erec))
            target[e], dist[e] = n, -1.0
            n += 1
            continue
        n_qual += 1
        n_dynamic += [dyn for c, _, dyn in qualifying if c == best_c][0]
        n_ties += any(c != best_c and dc == best for c, dc, _ in qualifying)
        for rec in erec:                                           # Scene::merge -> addOrigin, record level
            if not any(rec[0] == h[0] and rec[1] == h[1] and rec[2] == h[2] for h in records[best_c]):
                records[best_c].append(rec)
        target[e], dist[e] = best_c, best
    if stats is not None:
        stats.update(merged=n_qual, dynamic=n_dynamic, ties=n_ties)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in records])
    flat = [rec for r in records for rec in r]
    return dict(xyz=xyz[:n].copy(), origin_offsets=off, origin_shot=np.array([r[0] for r in flat], np.int32),
                origin_xy=np.array([[r[1], r[2]] for r in flat], F64).reshape(-1, 2), target=target, merge_distance=dist)
