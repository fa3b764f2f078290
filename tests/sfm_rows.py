"""The library's rows as the steps of tests/sfm_ref.py, through the existing Python mirrors: one row call per
reference call (relative pose and triangulation on the pair alone, merge / 3D-2D search over the whole
match graph as it is at that moment, sfmx.ba.solve for the adjustment).  What sfmx_sfm_triangulate must equal."""
import numpy as np

from sfmx import ba, pnp, pose, scene, triangulate
from sfmx.matching import DMATCH_DTYPE


class RowSteps:
    def __init__(self, keypoints, shot_size, camera, camera_model, pairs, matches, offsets, prm):
        self.kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
        self.n_shots = len(self.kps)
        self.size = np.asarray(shot_size, np.int32).reshape(-1, 2)
        self.K, self.dist = np.array(camera[0], np.float64).reshape(3, 3), np.array(camera[1], np.float64).reshape(5)
        self.model = camera_model
        self.pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        self.lists = [np.array(matches[offsets[p]:offsets[p + 1]], DMATCH_DTYPE) for p in range(len(self.pairs))]
        self.prm = prm
        self.sc = np.zeros(self.n_shots, np.int32)
        self.poses = np.full((self.n_shots, 3, 4), np.nan)
        self.xyz = np.zeros((0, 3))
        self.oo = np.zeros(1, np.int64)
        self.osh = np.zeros(0, np.int32)
        self.oxy = np.zeros((0, 2))
        self.ba_terminations = []

    def cams(self):
        return [(self.K, self.dist)]

    def graph(self):
        off = np.zeros(len(self.pairs) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in self.lists])
        return (np.concatenate(self.lists) if len(self.lists) else np.zeros(0, DMATCH_DTYPE)), off

    def relative_pose(self, p):
        lst = self.lists[p]
        r = pose.relative_poses(self.kps, self.cams(), self.sc, self.size, self.pairs[p:p + 1], lst, [0, len(lst)],
                                threshold=self.prm.ransac_baseline_threshold)
        if int(r["status"][0]) != 1:
            self.pend = None
            return 0, 0
        self.pend = (p, r["matches"].copy(), r["pose"][0].reshape(3, 4).copy())
        return 1, int(r["n_inliers"][0])

    def triangulate_pair(self, p, initial):
        assert self.pend is not None and self.pend[0] == p
        _, inl, rel = self.pend
        self.pend = None
        self.lists[p] = inl
        if initial:
            self.poses[self.pairs[p, 0]] = np.eye(3, 4)
            self.poses[self.pairs[p, 1]] = rel
        r = triangulate.triangulate_matches(self.kps, self.cams(), self.sc, self.poses, self.pairs[p:p + 1], inl, [0, len(inl)],
                                            max_reprojection_error=self.prm.max_reprojection_error)
        self.new = (r["xyz"].copy(), r["origin_shot"].copy(), r["origin_xy"].copy())
        return int(r["n_points"])

    def add_elements(self, p, merge):
        nx, ns, nxy = self.new
        if len(nx) == 0:
            return
        if not merge:
            self.xyz = np.concatenate([self.xyz, nx])
            self.oo = np.concatenate([self.oo, self.oo[-1] + 2 * np.arange(1, len(nx) + 1)])
            self.osh = np.concatenate([self.osh, ns])
            self.oxy = np.concatenate([self.oxy, nxy])
            return
        m, off = self.graph()
        r = scene.merge_pointcloud_3d2d(self.kps, self.pairs, m, off, self.xyz, self.oo, self.osh, self.oxy, nx,
                                        2 * np.arange(len(nx) + 1, dtype=np.int64), ns, nxy, self.prm.point_merge_distance,
                                        self.prm.feature_merge_distance)
        self.xyz, self.oo, self.osh, self.oxy = (r["xyz"].copy(), r["origin_offsets"].copy(), r["origin_shot"].copy(),
                                                 r["origin_xy"].copy())

    def count_candidates(self, shots):
        m, off = self.graph()   # SfM.cpp:278-282: one find3d2dMatches per remaining shot, the list sizes
        return [int((scene.find_3d2d_matches(self.kps, self.pairs, m, off, self.oo, self.osh, self.oxy, s)[0] >= 0).sum())
                for s in shots]

    def register_shot(self, shot):
        self.pend_shot = None
        if len(self.osh) == 0:
            return 0, -1.0, []
        m, off = self.graph()
        fk, fp, fxy = scene.find_3d2d_matches(self.kps, self.pairs, m, off, self.oo, self.osh, self.oxy, shot)
        p3, p2 = pnp.distinct_3d2d_points(self.xyz, self.oo, fk, fxy)
        distinct = []
        for p in fp[fk >= 0]:
            if int(p) not in distinct:
                distinct.append(int(p))
        if len(p3) == 0:
            return 0, -1.0, distinct
        r = pnp.register_poses(p3, p2, [0, len(p3)], [shot], self.cams(), self.sc, self.size,
                               threshold=self.prm.ransac_pose_threshold)
        status = int(r["status"][0])
        if status != 1:
            return status, -1.0, distinct
        self.pend_shot = (shot, r["pose"][0].reshape(3, 4).copy())
        return 1, float(r["inlier_ratio"][0]), distinct

    def accept_shot(self, shot):
        assert self.pend_shot[0] == shot
        self.poses[shot] = self.pend_shot[1]

    def bundle_adjust(self):
        if len(self.xyz) == 0:
            return 0, -1
        o = scene.ba_observations_from_origins(self.oo, self.osh, self.oxy, self.n_shots)
        sop = o["shot_of_pose"]
        f = self.K[0, 0] if self.K[0, 0] == self.K[1, 1] else (self.K[0, 0] + self.K[1, 1]) / 2.0
        intr = {ba.CAM_SIMPLE: [f], ba.CAM_SIMPLE_RADIAL: [f, self.dist[0], self.dist[1]],
                ba.CAM_DISTORTION: [f, self.K[0, 2], self.K[1, 2], *self.dist[:4]]}[self.model]
        pb = ba.BAProblem(self.model, self.xyz, np.array([ba.pose_to_ceres(self.poses[s]) for s in sop]), intr, o["obs_point"],
                          o["obs_cam"], o["obs_xy"], cx=self.K[0, 2], cy=self.K[1, 2])
        sm, _ = ba.solve(pb)
        self.xyz = pb.points.copy()
        for i, s in enumerate(sop):
            self.poses[s] = ba.pose_from_ceres(pb.poses[i]).reshape(3, 4)
        self.K[0, 0] = self.K[1, 1] = pb.intr[0]
        if self.model == ba.CAM_SIMPLE_RADIAL:
            self.dist[0], self.dist[1] = pb.intr[1], pb.intr[2]
        if self.model == ba.CAM_DISTORTION:
            self.K[0, 2], self.K[1, 2] = pb.intr[1], pb.intr[2]
            self.dist[:4] = pb.intr[3:7]
        self.ba_terminations.append(int(sm["termination_type"]))
        return int(sm["num_successful_steps"]) + int(sm["num_unsuccessful_steps"]), int(sm["termination_type"])
