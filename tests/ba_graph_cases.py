"""Camera co-visibility graphs that are not rings, and BA problems with a prescribed camera graph
(test infrastructure for tests/test_ba_masks.py and tests/test_gpu_ba_graphs.py).

On a banded graph (synth.ba_problem: every point seen by consecutive cameras) the nonzero 4-column
chunks of every A_ak of the block factorization are contiguous, so the row masks of ba_plan.cpp never
have a hole (a zero chunk between two set ones).  These graphs do."""
import numpy as np

from sfmx import synth


def _sym(C, pairs):
    a = np.zeros((C, C), np.uint8)
    for i, j in pairs:
        if i != j:
            a[i, j] = a[j, i] = 1
    return a


def ring(C, w):
    """Every camera with its w - 1 successors (a point seen by w consecutive cameras)."""
    return _sym(C, [(c, (c + d) % C) for c in range(C) for d in range(1, w)])


def skip_ring(C=48):
    """c ~ c + 3, c + 7, c + 10 (mod C): the union of the triangles {c, c + 3, c + 10}."""
    return _sym(C, [(c, (c + d) % C) for c in range(C) for d in (3, 7, 10)])


def hub_ring(C=40):
    """A ring of 3 (c ~ c + 1, c + 2) over the cameras 0 .. C - 2, and the hub camera C - 1 linked to
    every 4th of them."""
    n = C - 1
    return _sym(C, [(c, (c + d) % n) for c in range(n) for d in (1, 2)] + [(C - 1, c) for c in range(0, n, 4)])


RANDOM_SEED = 13   # connected, no isolated camera; 13 of the automatic plan's 29 src entries have a holed ka


def random_graph(C=60, p=0.06, seed=RANDOM_SEED):
    """Each pair with probability p (fixed seed; every camera has a neighbour: asserted)."""
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((C, C)) < p, 1)
    a = (up | up.T).astype(np.uint8)
    assert a.sum(1).min() >= 1, "a camera without a neighbour: choose another seed"
    return a


def chain_links(C=24):
    """The chain c ~ c + 1 plus the links 0-23, 5-23, 0-17."""
    return _sym(C, [(c, c + 1) for c in range(C - 1)] + [(0, 23), (5, 23), (0, 17)])


def two_clusters(n=15):
    """Two dense clusters of n cameras joined by two bridges."""
    pairs = [(i, j) for s in (0, n) for i in range(s, s + n) for j in range(i + 1, s + n)]
    return _sym(2 * n, pairs + [(3, n + 4), (n - 2, 2 * n - 1)])


def disconnected():
    """Three components, each a ring of 3 over 12 cameras."""
    return np.kron(np.eye(3, dtype=np.uint8), ring(12, 3))


HOLED = {"skip_ring": skip_ring, "hub_ring": hub_ring, "random": random_graph, "chain_links": chain_links}
OTHER = {"two_clusters": two_clusters, "disconnected": disconnected}
GRAPHS = dict(HOLED, **OTHER)


def spd_system(adj, plan, seed=0):
    """A random SPD S (generic values) with the camera-block pattern of adj in the plan's row layout and
    identity padding, and a right-hand side that is zero on the padding rows: the system
    tests/test_ba_plan.py simulate() builds.  -> (S, b, padding rows)."""
    rng = np.random.default_rng(seed)
    C, npad = adj.shape[0], plan["npad"]
    rows = plan["camrow"]
    M = np.zeros((npad, npad))
    for a in range(C):
        for b in range(a, C):
            if a == b or adj[a, b]:
                v = rng.normal(size=(6, 6))
                if a == b:
                    M[rows[a]:rows[a] + 6, rows[a]:rows[a] + 6] += v + v.T
                else:
                    M[rows[a]:rows[a] + 6, rows[b]:rows[b] + 6] += 0.3 * v
                    M[rows[b]:rows[b] + 6, rows[a]:rows[a] + 6] += 0.3 * v.T
    pad = np.ones(npad, bool)
    for c in range(C):
        pad[rows[c]:rows[c] + 6] = False
    M[np.ix_(~pad, ~pad)] += np.eye((~pad).sum()) * (np.abs(M).sum(1).max() + 1.0)   # diagonally dominant
    S = np.where(np.outer(pad, pad), np.eye(npad), M)
    return S, np.where(pad, 0.0, rng.normal(size=npad)), pad


def hull(m):
    """Every bit from the lowest to the highest set bit of m."""
    m = int(m)
    return 0 if m == 0 else ((1 << m.bit_length()) - 1) & ~((m & -m) - 1)


def has_hole(m):
    return hull(m) != int(m)


def view_sets(name, adj):
    """Cliques of the graph that cover every edge and nothing else: the triangles {c, c + 3, c + 10} of
    the skip ring, otherwise the edges."""
    C = adj.shape[0]
    if name == "skip_ring":
        sets = [tuple(sorted({c, (c + 3) % C, (c + 10) % C})) for c in range(C)]
    else:
        sets = [(i, j) for i in range(C) for j in range(i + 1, C) if adj[i, j]]
    cover = np.zeros_like(adj)
    for s in sets:
        for i in s:
            for j in s:
                if i != j:
                    cover[i, j] = 1
    assert np.array_equal(cover, adj), "the view sets must cover exactly the graph's edges"
    return sets


def problem(name, n_points, seed, cam_model=3):
    """synth.ba_problem with every camera seeing every point, cut down to the observations (point p,
    camera c) with c in p's view set; the view sets go round the points, so every edge of the graph
    gets points and every point keeps at least 2 views.  -> (BAProblem kwargs, adj)."""
    adj = GRAPHS[name]()
    C = adj.shape[0]
    sets = view_sets(name, adj)
    assert n_points >= len(sets)
    p = synth.ba_problem(C, n_points, obs_per_point=C, seed=seed, cam_model=cam_model)
    member = np.zeros((len(sets), C), bool)
    for i, s in enumerate(sets):
        member[i, list(s)] = True
    keep = member[p["obs_point"] % len(sets), p["obs_cam"]]
    out = dict(p, obs_point=p["obs_point"][keep], obs_cam=p["obs_cam"][keep], obs_xy=p["obs_xy"][keep])
    assert np.bincount(out["obs_point"], minlength=n_points).min() >= 2
    return out, adj
