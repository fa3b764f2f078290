"""A toy world for the control flow of SfM::triangulate: steps answered from tables instead of geometry.

Per pair a (status, inlier count) of the relative pose and a weight (the 3D-2D matches it carries); per shot a
(status, ratio) of the registration.  The world keeps what the steps own in the real scene (which shots have a
pose, which pairs put points into the cloud) and derives the candidate counts from it: the count of a shot is the
sum of the weights of the first pair in list order joining it with each shot that has points in the cloud, over
every pair of the scene (Scene::find3d2dMatches reads them all).  Every call is logged with its answer; the log
of a tests/sfm_ref.py run is what tests/cpp/sfm_host_main.cpp replays."""
import numpy as np

PARAMS = dict(min_match_count_for_baseline=100, min_homography_inlier_ratio=0.5, min_pose_inlier_ratio=0.5)


class Scenario:
    def __init__(self, name, n_shots, pairs, n_matches, homography, pose, weight, registration, params=None, stray=False):
        self.name = name
        self.n_shots = n_shots
        self.pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        n = len(self.pairs)
        self.n_matches = np.asarray(n_matches, np.int32).reshape(-1)
        self.homography = np.asarray(homography, np.float64).reshape(-1)
        self.pose = list(pose)                  # per pair (status, n_inliers)
        self.weight = list(weight)              # per pair
        self.registration = list(registration)  # per shot (status, ratio)
        self.params = dict(PARAMS, **(params or {}))
        self.stray = stray                      # register_shot also names the shot's pairs with shots outside the cloud
        assert len(self.n_matches) == n and len(self.homography) == n and len(self.pose) == n and len(self.weight) == n
        assert len(self.registration) == n_shots


class World:
    def __init__(self, sc: Scenario):
        self.sc = sc
        self.posed = set()     # shots with a pose
        self.in_cloud = set()  # shots that are an origin of a cloud point
        self.pending = None
        self.ba_calls = 0
        self.log = []          # (step, arguments..., answers...)

    def _first_pairs(self, shot):
        """other shot in the cloud -> first pair in list order joining {shot, other}"""
        first = {}
        for p, (l, r) in enumerate(self.sc.pairs):
            if l == r:
                continue
            o = int(r) if l == shot else (int(l) if r == shot else -1)
            if o >= 0 and o in self.in_cloud and o not in first:
                first[o] = p
        return first

    def relative_pose(self, pair):
        status, n = self.sc.pose[pair]
        self.log.append(("relative_pose", pair, status, n))
        return status, n

    def triangulate_pair(self, pair, initial):
        l, r = (int(v) for v in self.sc.pairs[pair])
        if initial:
            self.posed |= {l, r}
        assert l in self.posed and r in self.posed, "triangulation of a pair without both poses"
        n_points = self.sc.pose[pair][1] // 2
        self.pending = (pair, n_points)
        self.log.append(("triangulate_pair", pair, int(initial), n_points))
        return n_points

    def add_elements(self, pair, merge):
        assert self.pending is not None and self.pending[0] == pair, "add_elements without its triangulate_pair"
        if self.pending[1] > 0:
            self.in_cloud |= {int(v) for v in self.sc.pairs[pair]}
        self.pending = None
        self.log.append(("add_elements", pair, int(merge)))

    def count_candidates(self, shots):
        counts = [sum(self.sc.weight[p] for p in self._first_pairs(s).values()) for s in shots]
        self.log.append(("count_candidates", tuple(shots), tuple(counts)))
        return counts

    def register_shot(self, shot):
        status, ratio = self.sc.registration[shot]
        first = self._first_pairs(shot)
        if not first:
            status = 0     # no 3D-2D match at all: the pose estimation throws
        distinct = [p for p in sorted(first.values(), key=lambda p: (-self.sc.weight[p], p)) if self.sc.weight[p] > 0]
        if self.sc.stray:
            distinct += [p for p, (l, r) in enumerate(self.sc.pairs) if shot in (l, r) and p not in distinct]
        self.pending_shot = shot
        self.log.append(("register_shot", shot, status, ratio, tuple(distinct)))
        return status, ratio, distinct

    def accept_shot(self, shot):
        assert self.pending_shot == shot
        self.posed.add(shot)
        self.log.append(("accept_shot", shot))

    def bundle_adjust(self):
        self.ba_calls += 1
        it, term = 3 + self.ba_calls % 4, self.ba_calls % 2
        self.log.append(("bundle_adjust", it, term))
        return it, term


def _graph(name, n_shots, pairs, **kw):
    """Defaults: every pair has 200 matches, 150 inliers, weight by index; ratios ascend with the pair index;
    every registration succeeds."""
    n = len(pairs)
    d = dict(n_matches=[200] * n, homography=[0.6 + 0.01 * i for i in range(n)], pose=[(1, 150)] * n,
             weight=[10 + (7 * i) % 5 for i in range(n)], registration=[(1, 0.8)] * n_shots)
    d.update(kw)
    return Scenario(name, n_shots, pairs, **d)


def named_scenarios():
    chain = [(i, i + 1) for i in range(5)]
    ring = chain + [(5, 0)]
    complete = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    out = [_graph("chain6", 6, chain), _graph("ring6", 6, ring), _graph("complete6", 6, complete)]
    out.append(_graph("all_below_homography", 6, ring, homography=[0.1, 0.2, 0.3, 0.4, 0.45, 0.49999]))
    pose = [(1, 150)] * len(complete)
    pose[0] = (0, 0)      # first candidate: throws
    pose[1] = (1, 99)     # second: 99 / 200 < 0.5
    out.append(_graph("two_initial_rejected", 6, complete, pose=pose))
    nm = [200] * len(complete)
    for i in (0, 2, 3, 7):
        nm[i] = 40 + i    # below min_match_count_for_baseline, with the lowest ratios
    out.append(_graph("below_min_baseline_mixed", 6, complete, n_matches=nm,
                      pose=[(1, int(0.75 * m)) for m in nm]))
    out.append(_graph("ties", 6, complete, homography=[0.7] * len(complete), weight=[5] * len(complete)))
    reg = [(1, 0.8)] * 6
    reg[3] = (1, 0.2)
    out.append(_graph("one_registration_fails", 6, complete, registration=reg))
    reg = [(1, 0.8)] * 6
    reg[2] = (2, 0.9)     # the unbuilt P3P: status 2 counts as "throws"
    out.append(_graph("registration_status_2", 6, ring, registration=reg))
    out.append(_graph("every_registration_fails", 6, complete, registration=[(1, 0.3)] * 6))
    pose = [(1, 150)] * len(ring)
    pose[2] = (0, 0)      # inside the loop: the pair stays open
    out.append(_graph("pair_throws_in_loop", 6, ring, pose=pose))
    out.append(_graph("two_components", 6, [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5)]))
    out.append(_graph("stray_distinct_pairs", 6, complete, stray=True))
    out.append(_graph("two_shots", 2, [(0, 1)]))
    out.append(_graph("no_pairs", 3, []))
    out.append(_graph("empty_lists", 3, [(0, 1), (1, 2)], n_matches=[0, 0], pose=[(1, 0), (1, 0)]))
    out.append(_graph("repeated_and_reversed_pairs", 4, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (0, 3), (1, 1)]))
    return out


def random_scenarios(count=200, seed=20260117):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n_shots = int(rng.integers(3, 10))
        allp = [(i, j) for i in range(n_shots) for j in range(n_shots) if i != j]
        n_pairs = int(rng.integers(1, min(len(allp), 16) + 1))
        pairs = [allp[i] for i in rng.permutation(len(allp))[:n_pairs]]
        n_matches = rng.integers(20, 300, n_pairs)
        pose = [(int(rng.random() < 0.85), int(m * rng.choice([0.2, 0.5, 0.7, 0.9]))) for m in n_matches]
        out.append(Scenario(f"random{k}", n_shots, pairs, n_matches,
                            rng.choice([0.3, 0.5, 0.55, 0.6, 0.6, 0.7, 0.9], n_pairs),
                            pose, [int(v) for v in rng.integers(0, 4, n_pairs) * 5],
                            [(int(rng.choice([0, 1, 1, 1, 1, 2])), float(rng.choice([0.2, 0.5, 0.8, 1.0]))) for _ in range(n_shots)],
                            stray=bool(k % 2)))
    return out


def same_trace(a, b):
    """Equal event lists; float values compare as bit patterns (a NaN ratio equals itself)."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x[:3] != y[:3] or np.float64(x[3]).tobytes() != np.float64(y[3]).tobytes():
            return False
    return True
