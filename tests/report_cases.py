"""Case builders of the report tests (tests/test_report_*.py, tests/test_gpu_report.py,
tests/golden/make_report_golden.py): scenes as the arrays sfmx.report takes."""
import numpy as np

IMAGE_SIZES = ((64, 48), (37, 29), (5, 4), (40, 30), (33, 21))   # width, height per shot


def image(shot, width, height, pad=7):
    """An 8-bit BGR image whose pixels are pairwise distinct (b, g hold the pixel index), as a view of a buffer
    with `pad` spare bytes per row: the pitch is 3 * width + pad."""
    idx = np.arange(width * height, dtype=np.int64).reshape(height, width)
    buf = np.full((height, 3 * width + pad), 0xEE, np.uint8)
    pix = np.stack([idx & 255, (idx >> 8) | (shot << 4), (idx * 7 + shot) & 255], axis=2).astype(np.uint8)
    buf[:, :3 * width] = pix.reshape(height, 3 * width)
    view = np.lib.stride_tricks.as_strided(buf, (height, width, 3), (buf.strides[0], 3, 1), writeable=False)
    assert np.array_equal(view, pix)
    return view


def images(n_shots=5):
    return [image(s, *IMAGE_SIZES[s]) for s in range(n_shots)]


def ring_poses(n_shots, radius=4.0):
    """3x4 [R|t] of cameras on a ring looking at the origin."""
    out = np.zeros((n_shots, 3, 4))
    for c in range(n_shots):
        ang = 2 * np.pi * c / n_shots + 0.1
        C = np.array([radius * np.cos(ang), radius * np.sin(ang), 0.3 * np.sin(3 * ang)])
        z = -C / np.linalg.norm(C)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        out[c, :, :3] = R
        out[c, :, 3] = -R @ C
    return out


def two_cameras():
    """[(K, dist)]: one with k1 only, one with all five coefficients."""
    K0 = np.array([[120.0, 0, 32.0], [0, 120.0, 24.0], [0, 0, 1]])
    K1 = np.array([[118.5, 0, 30.25], [0, 121.75, 25.5], [0, 0, 1]])
    return [(K0, np.array([-0.11, 0, 0, 0, 0])), (K1, np.array([0.08, -0.03, 0.002, -0.001, 0.01]))]


def _project64(x, P, K, dist):
    Xc = P[:, :3] @ x + P[:, 3]
    a, b = Xc[0] / Xc[2], Xc[1] / Xc[2]
    r2 = a * a + b * b
    k1, k2, p1, p2, k3 = dist
    cd = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return np.array([(a * cd + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)) * K[0, 0] + K[0, 2],
                     (b * cd + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b) * K[1, 1] + K[1, 2]])


def scene(counts, seed, n_shots=5, noise=0.75, float_points=False):
    """A cloud with counts[p] origin records at point p: shots drawn at random (repeats allowed), positions the
    projection plus pixel noise.  float_points: coordinates that are float32 values."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    xyz = rng.uniform(-0.6, 0.6, (n, 3))
    if float_points:
        xyz = xyz.astype(np.float32).astype(np.float64)
    cams = two_cameras()
    shot_camera = np.array([0, 1, 0, 1, 1][:n_shots], np.int32) if n_shots <= 5 else (np.arange(n_shots) % 2).astype(np.int32)
    poses = ring_poses(n_shots)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    m = int(off[-1])
    osh = rng.integers(0, n_shots, m).astype(np.int32)
    pt = np.repeat(np.arange(n), counts)
    oxy = np.zeros((m, 2))
    for i in range(m):
        K, dist = cams[shot_camera[osh[i]]]
        oxy[i] = _project64(xyz[pt[i]], poses[osh[i]], K, dist)
    oxy += rng.normal(0, noise, oxy.shape)
    return dict(xyz=xyz, origin_offsets=off, origin_shot=osh, origin_xy=oxy, cameras=cams, shot_camera=shot_camera,
                shot_pose=poses.reshape(n_shots, 12))


def golden_counts():
    """About 300 points with 0 to 7 records; empty rows at the start, in the middle and at the end; one point
    with 300 records."""
    c = np.random.default_rng(2024).integers(0, 8, 301)
    c[0] = c[1] = c[150] = c[151] = c[-1] = c[-2] = 0
    c[77] = 300
    return c


def golden_scene():
    return scene(golden_counts(), 31)


def from_golden(g):
    """The scene dict, the images (padded rows, the golden file's pixels), the camera and shot lists of the
    camera PLY from tests/golden/report_small.npz as fixtures.load returns it."""
    sc = dict(xyz=g["xyz"], origin_offsets=g["origin_offsets"], origin_shot=g["origin_shot"], origin_xy=g["origin_xy"],
              cameras=[(K, d) for K, d in zip(g["cam_K"], g["cam_dist"])], shot_camera=g["shot_camera"], shot_pose=g["shot_pose"])
    ims = images(5)
    for i, im in enumerate(ims):
        assert np.array_equal(im, g["image%d" % i])
    cams = [(int(w), int(h), K) for (w, h), K in zip(g["cam_size"], g["cam_K"])]
    return sc, ims, cams, mvs_shots(sc, [bool(v) for v in g["recovered"]])


def sized_scene(n_origins, seed=5):
    """Exactly n_origins records: three per point, the last point the rest."""
    full, rest = divmod(n_origins, 3)
    return scene([3] * full + ([rest] if rest else []), seed)


def args(sc):
    return (sc["xyz"], sc["origin_offsets"], sc["origin_shot"], sc["origin_xy"], sc["cameras"], sc["shot_camera"], sc["shot_pose"])


def mvs_cameras(sc, sizes=((64, 48), (48, 64))):
    """[(width, height, K)] of the scene's cameras: a landscape and a portrait one."""
    return [(w, h, K) for (w, h), (K, _) in zip(sizes, sc["cameras"])]


def mvs_shots(sc, recovered=None):
    n = len(sc["shot_camera"])
    rec = [True] * n if recovered is None else recovered
    return [(int(sc["shot_camera"][i]), bool(rec[i]), sc["shot_pose"][i]) for i in range(n)]


def degenerate_scene():
    """One shot [I|0] with the k1 camera.  Points: on the camera plane (z == 0: the z = 1 rule), NaN, +inf and
    -inf coordinates, a coordinate beyond the float range, an ordinary point whose record position is NaN, an
    ordinary point."""
    cams = two_cameras()[:1]
    xyz = np.array([[0.5, 0.25, 0.0], [np.nan, 0.1, 2.0], [0.1, np.inf, 2.0], [0.1, 0.2, -np.inf], [1e300, 0.2, 2.0],
                    [0.1, 0.2, 2.0], [0.1, -0.2, 3.0]])
    off = np.arange(len(xyz) + 1, dtype=np.int64)
    oxy = np.array([[30.0, 20.0]] * len(xyz))
    oxy[5] = (np.nan, 20.0)
    pose = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12)
    return dict(xyz=xyz, origin_offsets=off, origin_shot=np.zeros(len(xyz), np.int32), origin_xy=oxy, cameras=cams,
                shot_camera=np.zeros(1, np.int32), shot_pose=pose)


def colour_case():
    """Three shots with images 64x48, 37x29, 5x4.  -> (n_points, offsets, shots, positions, images)."""
    rows = [
        [(0, 2.5, 3.5)],                       # half-integers on both parities: 2, 4
        [(0, 3.5, 2.5)],                       # 4, 2
        [(0, -0.4, 0.0)],                      # -0.0 -> 0: inside
        [(0, -0.5, 5.0)],                      # -0.5 -> -0 -> 0: inside
        [(0, -0.6, 5.0)],                      # -1: outside
        [(0, 63.5, 1.0)],                      # w - 0.5, w even: 64 -> outside
        [(1, 36.5, 1.0)],                      # w - 0.5, w odd: 36 -> inside
        [(0, 5.0, 47.5)],                      # h - 0.5, h even: 48 -> outside
        [(1, 5.0, 28.5)],                      # h - 0.5, h odd: 28 -> inside
        [(2, np.nan, 1.0)],                    # NaN: default, record named
        [(2, 1.0, np.inf)],
        [],                                    # no record
        [(2, 1.0, 1.0), (1, 7.0, 8.0), (2, 2.0, 2.0), (0, 9.0, 9.0), (0, 10.0, 10.0)],   # the lowest shot comes late, and twice
        [(1, 3.0, 3.0), (2, 4.0, 3.0), (1, 5.0, 5.0)],
        [(2, 4.49, 3.5)],                      # 4, 4: the last pixel of the 5x4 image?  (4, 4) is outside: h = 4
        [(2, 4.49, 3.49)],                     # (4, 3): the last pixel
        [(0, 1e300, 1.0)],                     # finite, far outside
        [(0, -3e9, 1.0)],
    ]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [t for r in rows for t in r]
    osh = np.array([t[0] for t in flat], np.int32)
    oxy = np.array([[t[1], t[2]] for t in flat], np.float64)
    return len(rows), off, osh, oxy, images(3)
